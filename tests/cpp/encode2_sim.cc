// Test harness (not product code): a key frame encoded in TWO passes on the host, as aa_encode_two_pass_batch's kernels do it -- the first
// pass under KeyPolicy (what encode_sim.cc runs), what it leaves behind (key2_first_pass.hh: the side bits, the branch counts and their
// token_prob_update), the second pass under Key2Policy (reencode_mb.hh over trellis_quant.hh), its own update merged over the first's.
// `Lanes` = sixteen register files and a loop; macroblocks in raster order where the kernels walk anti-diagonals.  Built by
// tests/test_encode2_sim.py with plain g++:
//   g++ -shared encode2_sim.cc                              the library the tests compare field by field
//   g++ -DENCODE2_SIM_MAIN -fsanitize=... encode2_sim.cc    a stand-alone program over case files: inputs, then what the reference wrote
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alfalfa_amd/csrc/reencode_mb.hh"
#include "../../alfalfa_amd/csrc/key2_first_pass.hh"

namespace {
struct HostLanes {
  using Regs = aa::ReencRegs2;
  Regs r[16];
  template <class F> void each( F f ) { for ( int b = 0; b < 16; b++ ) f( b, r[b] ); }
  template <class F> uint32_t sum( F f ) { uint32_t t = 0; for ( int b = 0; b < 16; b++ ) t += f( b, r[b] ); return t; }
  template <class F> int32_t sumi( F f ) { int32_t t = 0; for ( int b = 0; b < 16; b++ ) t += f( b, r[b] ); return t; }
  void sync() {}
};

template <class P>
void walk( const aa_reencode_dev_job & J, size_t nmb )
{
  for ( size_t mi = 0; mi < nmb; mi++ ) {
    aa::ReencLds S;
    std::memset( &S, 0, sizeof S );
    static HostLanes lanes;
    std::memset( static_cast<void *>( &lanes ), 0, sizeof lanes );
    aa::ReencMb<HostLanes, P> mb( lanes, J, S, mi );
    mb.run();
  }
}

// the branch counts of a pass's raw output -> its 1056 update flags and 1056 values against the default tables
void updates_of( const aa_mb_info * recs, const uint32_t * masks, const int16_t * dense, int mbw, size_t nmb, uint8_t * updates )
{
  std::vector<uint32_t> counts( 2112, 0 );
  for ( size_t mi = 0; mi < nmb; mi++ )
    for ( uint32_t b = 0; b < 24; b++ )
      aa::count_raw_block( [&]( const uint32_t node, const uint32_t taken ) { counts[2 * node + taken]++; }, recs, masks, dense, static_cast<uint32_t>( mbw ), static_cast<uint32_t>( mi ), b );
  for ( int i = 0; i < 1056; i++ ) aa::key_update( counts[2 * i], counts[2 * i + 1], k_default_coeff_probs[i], updates[i], updates[1056 + i] );
}
}

extern "C" {

enum { CENSUS_MODE_CHANGED = aa::K2_CENSUS, CENSUS_FIELD_SURVIVES, CENSUS_WORDS };
int encode2_sim_census_words() { return CENSUS_WORDS; }

// One key frame in two passes.  target: padded planes Y, U, V one after the other (stride = padded width); quant: {y_dc, y_ac, y2_dc,
// y2_ac, uv_dc, uv_ac}.  Out: mbs / dense / recon as encode_sim_frame's, of the SECOND pass; first_mbs (may be null): the first pass's
// records; updates: 1056 flags then 1056 values, the header's token_prob_update after both passes; census[CENSUS_WORDS]: how often each
// case the fixtures are meant to hold was met (reencode_search.hh K2_*, then macroblocks whose mode changed between the passes and header
// fields that survive from the first pass).  scrub != 0: the reconstruction raster is overwritten between the passes -- the second pass
// reads no pixel the first one wrote, so nothing may change.  first_updates_out (may be null): the FIRST pass's 1056 flags then 1056
// values, before the merge -- what aa_encode_two_pass_batch hands back for the serialiser.
int encode2_sim_frame_first( int mbw, int mbh, const uint8_t * target, const uint16_t quant[6], aa_mb_info * mbs, int16_t * dense, uint8_t * recon, aa_mb_info * first_mbs,
                             uint8_t * updates, uint32_t * census, int scrub, uint8_t * first_updates_out )
{
  const size_t nmb = size_t( mbw ) * mbh, ysz = nmb * 256, csz = nmb * 64;
  std::vector<uint32_t> masks( nmb, 0 ), nb( nmb * 4, 0 );
  aa_reencode_dev_job J;
  std::memset( &J, 0, sizeof J );
  J.base.target[0] = target; J.base.target[1] = target + ysz; J.base.target[2] = target + ysz + csz;
  J.base.target_stride[0] = mbw * 16; J.base.target_stride[1] = mbw * 8;
  J.base.recon[0] = recon; J.base.recon[1] = recon + ysz; J.base.recon[2] = recon + ysz + csz;
  J.base.coeffs = dense; J.base.masks = masks.data();
  std::memcpy( J.base.quant, quant, sizeof J.base.quant );
  J.base.mbw = static_cast<uint16_t>( mbw ); J.base.mbh = static_cast<uint16_t>( mbh ); J.base.has_intra = 1;
  J.mbs_out = mbs; J.nb = nb.data();
  // ---- the first pass, and what it leaves ----
  aa::EncKey2Costs C;
  std::memset( &C, 0, sizeof C );
  aa::enc_fill_key_costs( C.enc, quant[1] );
  J.costs = &C.enc;
  walk<aa::KeyPolicy>( J, nmb );
  std::vector<uint8_t> bits( nmb ), first_updates( 2112 );
  std::vector<uint8_t> first_modes( nmb );
  for ( size_t mi = 0; mi < nmb; mi++ ) { bits[mi] = aa::first_pass_bits( mbs[mi], masks[mi] ); first_modes[mi] = mbs[mi].y_mode; }
  if ( first_mbs ) std::memcpy( first_mbs, mbs, nmb * sizeof( aa_mb_info ) );
  updates_of( mbs, masks.data(), dense, mbw, nmb, first_updates.data() );
  if ( first_updates_out ) std::memcpy( first_updates_out, first_updates.data(), 2112 );
  if ( scrub ) std::memset( recon, 0x5A, nmb * 384 );
  // ---- the second pass ----
  static aa::TrellisCosts T;
  aa::trellis_fill_costs( T );
  std::vector<uint32_t> met( CENSUS_WORDS, 0 );
  C.trellis = &T; C.first_pass = bits.data(); C.census = met.data();
  J.costs = &C;
  walk<aa::Key2Policy>( J, nmb );
  updates_of( mbs, masks.data(), dense, mbw, nmb, updates );
  for ( int i = 0; i < 1056; i++ ) {
    if ( !updates[i] && first_updates[i] ) met[CENSUS_FIELD_SURVIVES]++;
    aa::merge_update( updates[i], updates[1056 + i], first_updates[i], first_updates[1056 + i] );
  }
  for ( size_t mi = 0; mi < nmb; mi++ ) {
    if ( mbs[mi].y_mode != first_modes[mi] ) met[CENSUS_MODE_CHANGED]++;
    for ( int b = 0; b < 25; b++ ) if ( !( ( masks[mi] >> b ) & 1u ) || ( b == 24 && mbs[mi].y_mode == aa::B_PRED ) ) std::memset( dense + ( mi * 25 + b ) * 16, 0, 32 );
    mbs[mi].nz_mask = aa::raw_context_mask( mbs[mi], masks[mi] );
  }
  if ( census ) std::memcpy( census, met.data(), CENSUS_WORDS * sizeof( uint32_t ) );
  return 0;
}

int encode2_sim_frame( int mbw, int mbh, const uint8_t * target, const uint16_t quant[6], aa_mb_info * mbs, int16_t * dense, uint8_t * recon, aa_mb_info * first_mbs,
                       uint8_t * updates, uint32_t * census, int scrub )
{
  return encode2_sim_frame_first( mbw, mbh, target, quant, mbs, dense, recon, first_mbs, updates, census, scrub, nullptr );
}

} // extern "C"

#if defined( ENCODE2_SIM_MAIN )
// case file: int32 mbw, mbh; uint16 quant[6]; target planes; then the reference's records [nmb], dense coefficients [nmb][25][16] and the
// 2112 bytes of its header's token_prob_update
int main( int argc, char ** argv )
{
  int bad = 0;
  for ( int a = 1; a < argc; a++ ) {
    FILE * f = std::fopen( argv[a], "rb" );
    if ( !f ) { std::fprintf( stderr, "%s: cannot open\n", argv[a] ); return 2; }
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    for ( size_t n; ( n = std::fread( buf, 1, sizeof buf, f ) ) > 0; ) d.insert( d.end(), buf, buf + n );
    std::fclose( f );
    int32_t h[2]; uint16_t quant[6];
    if ( d.size() < 20 ) { std::fprintf( stderr, "%s: short file\n", argv[a] ); return 2; }
    std::memcpy( h, d.data(), 8 ); std::memcpy( quant, d.data() + 8, 12 );
    const size_t nmb = size_t( h[0] ) * h[1], planes = nmb * 384;
    if ( h[0] <= 0 || h[1] <= 0 || d.size() != 20 + planes + nmb * ( sizeof( aa_mb_info ) + 800 ) + 2112 ) { std::fprintf( stderr, "%s: not a case file\n", argv[a] ); return 2; }
    const uint8_t * target = d.data() + 20;
    const uint8_t * want_mb = target + planes;
    const uint8_t * want_dense = want_mb + nmb * sizeof( aa_mb_info );
    const uint8_t * want_updates = want_dense + nmb * 800;
    std::vector<aa_mb_info> mbs( nmb );
    std::vector<int16_t> dense( nmb * 400 );
    std::vector<uint8_t> recon( planes ), updates( 2112 );
    encode2_sim_frame( h[0], h[1], target, quant, mbs.data(), dense.data(), recon.data(), nullptr, updates.data(), nullptr, 0 );
    size_t differ = 0;
    for ( size_t mi = 0; mi < nmb; mi++ ) {
      aa_mb_info w;
      std::memcpy( &w, want_mb + mi * sizeof w, sizeof w );
      const bool same = mbs[mi].y_mode == w.y_mode && mbs[mi].uv_mode == w.uv_mode && mbs[mi].ref_frame == w.ref_frame && mbs[mi].nz_mask == w.nz_mask
                        && !std::memcmp( &mbs[mi].u, &w.u, sizeof w.u ) && !std::memcmp( dense.data() + mi * 400, want_dense + mi * 800, 800 );
      if ( !same ) differ++;
    }
    const bool header = !std::memcmp( updates.data(), want_updates, 2112 );
    std::printf( "%s: %zu of %zu macroblocks differ from the reference; token_prob_update %s\n", argv[a], differ, nmb, header ? "equal" : "DIFFERS" );
    bad += differ != 0 || !header;
  }
  return bad ? 1 : 0;
}
#endif
