// The compaction of a re-encoded frame's records as k_reencode_count and k_reencode_compact (alfalfa_amd/csrc/reencode_compact_kernels.hip,
// compact_device.hh) state it, on the host and one thread at a time: reencode_compact.hh and rebase_compact.hh compiled for the host,
// workgroups of kCompactMbs threads over runs of as many macroblocks -- the count pass with its intra-row words (thread mi of the frame
// makes word mi), the wave reduction and the wave scan written as the shuffles do them, a word per run between the two passes, the record
// with its loop-filter level, the copy of the slots in 16-byte units with thread t taking units t, t + 256, ... -- and then what
// aa_reencode_device_batch derives from the words on the host: intra count and diagonals.  tests/test_reencode_compact_model.py compares
// what comes out with a plain transcription of reencode_records and the row / diagonal / count loops.
//
//   g++ -O2 -fPIC -shared                        -> reencode_compact_run() for ctypes
//   g++ -DREENCODE_COMPACT_MAIN -fsanitize=...   -> a program over case files: mbw, mbh, expected blocks, expected intra, filter parameters,
//                                                   then records, masks, dense slots, expected records, rows, diagonals, blocks' coefficients
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../alfalfa_amd/csrc/reencode_compact.hh"

namespace {

using namespace aa::compact;
constexpr uint32_t kWave = 64, kWaves = kCompactMbs / kWave;

// __shfl_down / __shfl_up over one wave: a lane whose source lies outside the wave gets its own value back
uint32_t shfl_down( const uint32_t * v, uint32_t lane, uint32_t off ) { return lane + off < kWave ? v[lane + off] : v[lane]; }
uint32_t shfl_up( const uint32_t * v, uint32_t lane, uint32_t off ) { return lane >= off ? v[lane - off] : v[lane]; }

// k_reencode_count, one workgroup: the run's sum, and the row words whose number is a macroblock of this run
uint32_t count_run( const aa_mb_info * in, const uint32_t * masks, uint32_t mbw, uint32_t mbh, uint32_t run, unsigned long long * rows )
{
  uint32_t n[kCompactMbs], wave_sum[kWaves];
  const uint32_t nmb = mbw * mbh, first = run * kCompactMbs;
  for ( uint32_t t = 0; t < kCompactMbs; t++ ) {
    const uint32_t mi = first + t;
    if ( mi < row_words( mbw, mbh ) ) rows[mi] = intra_row_word( in, mbw, mi );
    n[t] = mi < nmb ? popc( stored_mask( masks[mi], in[mi].y_mode ) ) : 0u;
  }
  for ( uint32_t w = 0; w < kWaves; w++ ) {
    uint32_t * v = n + w * kWave;
    for ( uint32_t off = 32; off; off >>= 1 ) {
      uint32_t next[kWave];
      for ( uint32_t l = 0; l < kWave; l++ ) next[l] = v[l] + shfl_down( v, l, off );
      std::memcpy( v, next, sizeof next );
    }
    wave_sum[w] = v[0];
  }
  uint32_t sum = 0;
  for ( uint32_t w = 0; w < kWaves; w++ ) sum += wave_sum[w];
  return sum;
}

// k_reencode_compact, one workgroup.  -> false: a unit would be stored outside the frame's blocks
bool compact_run( const aa_mb_info * in, const uint32_t * masks, const int16_t * dense, uint32_t nmb, const uint32_t * partials, uint32_t run, const aa::HeaderParams & fp,
                  aa_mb_info * out, int16_t * coeffs_out, uint32_t num_blocks )
{
  uint32_t run_mask[kCompactMbs], run_index[kCompactMbs], n[kCompactMbs], incl[kCompactMbs], wave_sum[kWaves];
  const uint32_t first = run * kCompactMbs;
  const uint32_t in_run = nmb - first < kCompactMbs ? nmb - first : kCompactMbs;
  const uint32_t base = run_base( partials, run );
  for ( uint32_t t = 0; t < kCompactMbs; t++ ) {
    const uint32_t mi = first + t;
    run_mask[t] = mi < nmb ? stored_mask( masks[mi], in[mi].y_mode ) : 0u;
    n[t] = incl[t] = popc( run_mask[t] );
  }
  for ( uint32_t w = 0; w < kWaves; w++ ) {
    uint32_t * v = incl + w * kWave;
    for ( uint32_t off = 1; off < kWave; off <<= 1 ) {
      uint32_t next[kWave];
      for ( uint32_t l = 0; l < kWave; l++ ) { const uint32_t got = shfl_up( v, l, off ); next[l] = l >= off ? v[l] + got : v[l]; }
      std::memcpy( v, next, sizeof next );
    }
    wave_sum[w] = v[kWave - 1];
  }
  for ( uint32_t t = 0; t < kCompactMbs; t++ ) {
    uint32_t before = base;
    for ( uint32_t w = 0; w < kWaves; w++ ) if ( w < t / kWave ) before += wave_sum[w];
    run_index[t] = before + incl[t] - n[t];
    const uint32_t mi = first + t;
    if ( mi < nmb ) out[mi] = reencode_record( in[mi], masks[mi], run_index[t], fp );
  }
  const uint8_t * src = reinterpret_cast<const uint8_t *>( dense ) + static_cast<size_t>( first ) * kSlots * 32;
  uint8_t * dst = reinterpret_cast<uint8_t *>( coeffs_out );
  const uint32_t units = in_run * kUnitsPerMb;
  for ( uint32_t t = 0; t < kCompactMbs; t++ )
    for ( uint32_t u = t; u < units; u += kCompactMbs ) {
      const Unit x = unit_of( u );
      const uint32_t m = run_mask[x.mb];
      if ( !unit_stored( x, m ) ) continue;
      const uint32_t block = unit_block( x, m, run_index[x.mb] );
      if ( block >= num_blocks ) return false;
      std::memcpy( dst + static_cast<size_t>( block ) * 32 + x.half * 16, src + unit_source( x ), 16 );
    }
  return true;
}

} // namespace

// The filter parameters as the caller has them: lf[0] the header's level, lf[1] != 0: adjustments on, lf[2..5] by reference, lf[6..9] by mode
// count -> sum, intra count and diagonals on the "host" -> compact.  rows: row_words words; diagonals: mbw + 2 * (mbh - 1) bytes.
// -> 0, 1: more blocks than coeffs_out holds (capacity_blocks), 2: a unit aimed outside the frame's blocks
extern "C" int reencode_compact_run( const aa_mb_info * in, const uint32_t * masks, const int16_t * dense, uint32_t mbw, uint32_t mbh, const int8_t * lf, aa_mb_info * out,
                                     int16_t * coeffs_out, uint32_t capacity_blocks, uint32_t * num_blocks, unsigned long long * rows, uint32_t * num_intra, uint8_t * diagonals )
{
  const uint32_t nmb = mbw * mbh, runs = runs_of( nmb );
  aa::HeaderParams fp;
  lf_params( fp, static_cast<uint8_t>( lf[0] ), lf[1] != 0, lf + 2, lf + 6 );
  std::vector<uint32_t> partials( runs );
  for ( uint32_t r = 0; r < runs; r++ ) partials[r] = count_run( in, masks, mbw, mbh, r, rows );
  uint32_t total = 0;
  for ( uint32_t r = 0; r < runs; r++ ) total += partials[r];
  *num_blocks = total;
  *num_intra = intra_count( rows, row_words( mbw, mbh ) );
  std::memset( diagonals, 0, mbw + 2 * ( mbh - 1 ) );
  intra_diagonals( rows, mbw, mbh, diagonals );
  if ( total > capacity_blocks ) return 1;
  for ( uint32_t r = 0; r < runs; r++ ) if ( !compact_run( in, masks, dense, nmb, partials.data(), r, fp, out, coeffs_out, total ) ) return 2;
  return 0;
}

#ifdef REENCODE_COMPACT_MAIN
int main( int argc, char ** argv )
{
  int bad = 0;
  for ( int a = 1; a < argc; a++ ) {
    FILE * f = std::fopen( argv[a], "rb" );
    uint32_t head[4];
    int8_t lf[12];
    if ( !f || std::fread( head, 4, 4, f ) != 4 || std::fread( lf, 1, 12, f ) != 12 ) { std::fprintf( stderr, "%s: cannot read\n", argv[a] ); return 2; }
    const uint32_t mbw = head[0], mbh = head[1], want_blocks = head[2], want_intra = head[3], nmb = mbw * mbh;
    const uint32_t words = row_words( mbw, mbh ), ndiag = mbw + 2 * ( mbh - 1 );
    std::vector<aa_mb_info> in( nmb ), want( nmb ), out( nmb );
    std::vector<uint32_t> masks( nmb );
    std::vector<unsigned long long> want_rows( words ), rows( words );
    std::vector<uint8_t> want_diag( ndiag ), diag( ndiag );
    const size_t shorts = size_t( want_blocks ) * 16;
    std::vector<int16_t> dense( size_t( nmb ) * kSlots * 16 ), want_coeffs( shorts + 16 ), coeffs( shorts + 16 );      // (never empty: a frame may store nothing)
    const bool ok = std::fread( in.data(), sizeof( aa_mb_info ), nmb, f ) == nmb && std::fread( masks.data(), 4, nmb, f ) == nmb
                    && std::fread( dense.data(), 2, dense.size(), f ) == dense.size() && std::fread( want.data(), sizeof( aa_mb_info ), nmb, f ) == nmb
                    && std::fread( want_rows.data(), 8, words, f ) == words && std::fread( want_diag.data(), 1, ndiag, f ) == ndiag
                    && std::fread( want_coeffs.data(), 2, shorts, f ) == shorts;
    std::fclose( f );
    if ( !ok ) { std::fprintf( stderr, "%s: short file\n", argv[a] ); return 2; }
    uint32_t blocks = 0, intra = 0;
    const int rc = reencode_compact_run( in.data(), masks.data(), dense.data(), mbw, mbh, lf, out.data(), coeffs.data(), want_blocks, &blocks, rows.data(), &intra, diag.data() );
    if ( rc || blocks != want_blocks || intra != want_intra || std::memcmp( out.data(), want.data(), nmb * sizeof( aa_mb_info ) )
         || std::memcmp( rows.data(), want_rows.data(), words * 8 ) || std::memcmp( diag.data(), want_diag.data(), ndiag )
         || std::memcmp( coeffs.data(), want_coeffs.data(), coeffs.size() * 2 ) ) {
      std::fprintf( stderr, "%s: status %d, %u blocks (want %u), %u intra (want %u), or records, words, diagonals or coefficients differ\n", argv[a], rc, blocks, want_blocks, intra, want_intra );
      bad++;
    }
  }
  std::printf( "%d cases, %d bad\n", argc - 1, bad );
  return bad ? 1 : 0;
}
#endif
