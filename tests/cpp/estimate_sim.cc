// Test harness (not product code): the frame-size estimate and the target-size search on the host, whole frames at a time.  It compiles the
// product's own headers -- reencode_search.hh (EstimateKeyPolicy, EstimateInterPolicy), reencode_mb.hh (one macroblock by sixteen lanes,
// kSampled), estimate_size.hh (the token walk that counts), qi_choose.hh (the rule) -- with `Lanes` = sixteen register files and a loop,
// walks the small frame's macroblocks in raster order where k_estimate_key / k_estimate_inter walk their anti-diagonals, and takes the
// size through the host path the runtime takes (serializer.cpp: estimate_frame_bytes).  The four pixels per macroblock row that no
// estimate writes (the policy's unwritten_pixels, reencode_search.hh) are zero in the product; here two derived policies put other values
// there, which is how the tests find the frames whose estimate does not depend on them.  Built by tests/test_estimate_sim.py with plain g++:
//   g++ -shared estimate_sim.cc parser.cpp serializer.cpp                        the library the tests call
//   g++ -DESTIMATE_SIM_MAIN -fsanitize=... estimate_sim.cc parser.cpp ...        a stand-alone program over case files
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alfalfa_amd/csrc/reencode_mb.hh"
#include "../../alfalfa_amd/csrc/estimate_size.hh"
#include "../../alfalfa_amd/csrc/qi_choose.hh"
#include "../../alfalfa_amd/csrc/serializer.hh"

namespace {
// the product's two policies with other values in the pixels no estimate writes
int g_fill = 0;        // 0: zeros (the product), 1: 255, 2 / 3: two seeded patterns that change from row to row
uint32_t unwritten_fill( int row )
{
  if ( g_fill == 0 ) return 0u;
  if ( g_fill == 1 ) return 0xFFFFFFFFu;
  uint32_t x = static_cast<uint32_t>( g_fill ) * 2654435761u + static_cast<uint32_t>( row ) * 40503u + 12345u;
  x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16;
  return x;
}
struct FilledKeyPolicy : aa::EstimateKeyPolicy { static uint32_t unwritten_pixels( const Costs &, int row ) { return unwritten_fill( row ); } };
struct FilledInterPolicy : aa::EstimateInterPolicy { static uint32_t unwritten_pixels( const Costs &, int row ) { return unwritten_fill( row ); } };

struct HostLanes {
  aa::ReencRegs r[16];
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
    HostLanes lanes;
    std::memset( &lanes, 0, sizeof lanes );
    aa::ReencMb<HostLanes, P> mb( lanes, J, S, mi );
    mb.run();
  }
}
}

extern "C" {

void estimate_sim_small_size( int w, int h, int out[4] )
{
  out[0] = w / 4; out[1] = h / 4; out[2] = ( w / 4 + 15 ) / 16; out[3] = ( h / 4 + 15 ) / 16;
}

// One estimate.  key != 0: a key estimate (ref, probs_before unused, may be null; carry untouched).  w, h: the picture's display size;
// ref / target: the padded planes Y, U, V of the ORIGINAL's size one after the other (stride = padded width); q_index: y_ac_qi, quant its
// factors; quality: 0 best, 1 real-time; probs_before: the stream's 1101 bytes before the frame; carry: {prob_inter, prob_references_last,
// prob_references_golden, vector costs filled}, bytes 0..2 in and out; fill: the pattern of the unwritten pixels.
// Out: size (the estimate: frame bytes * 16), mbs (y_mode, uv_mode, ref_frame, nz_mask, u of the small frame), dense [nmb][25][16] with zeros
// in every slot the mask leaves out; either may be null.  -> 0, or -1 for a picture under 4 pixels.
int estimate_sim( int key, int w, int h, const uint8_t * ref, const uint8_t * target, int q_index, const uint16_t quant[6], int quality, const uint8_t * probs_before,
                  uint8_t carry[4], int fill, uint64_t * size, aa_mb_info * mbs_out, int16_t * dense_out )
{
  if ( w / 4 < 1 || h / 4 < 1 ) return -1;
  const int fmbw = ( w + 15 ) / 16, fmbh = ( h + 15 ) / 16;
  const int mbw = ( w / 4 + 15 ) / 16, mbh = ( h / 4 + 15 ) / 16;
  const size_t nmb = size_t( mbw ) * mbh, fy = size_t( fmbw ) * fmbh * 256, fc = fy / 4;
  std::vector<uint32_t> masks( nmb, 0 ), nb( nmb * 4, 0 );
  std::vector<aa_mb_info> mbs( nmb );
  std::memset( mbs.data(), 0, nmb * sizeof( aa_mb_info ) );
  std::vector<int16_t> dense( nmb * 400, 0 );
  std::vector<uint8_t> recon( nmb * 384, 0 );
  aa_reencode_dev_job J;
  std::memset( &J, 0, sizeof J );
  if ( !key ) { J.base.ref[1][0] = ref; J.base.ref[1][1] = ref + fy; J.base.ref[1][2] = ref + fy + fc; }
  J.base.target[0] = target; J.base.target[1] = target + fy; J.base.target[2] = target + fy + fc;
  J.base.target_stride[0] = fmbw * 16; J.base.target_stride[1] = fmbw * 8;
  J.base.recon[0] = recon.data(); J.base.recon[1] = recon.data() + nmb * 256; J.base.recon[2] = recon.data() + nmb * 320;
  J.base.coeffs = dense.data(); J.base.masks = masks.data();
  std::memcpy( J.base.quant, quant, sizeof J.base.quant );
  J.base.mbw = static_cast<uint16_t>( mbw ); J.base.mbh = static_cast<uint16_t>( mbh ); J.base.has_intra = 1;
  J.mbs_out = mbs.data(); J.nb = nb.data();
  g_fill = fill;
  aa::ProbTables defaults;
  defaults.set_defaults();
  const uint8_t * token_probs = key ? &defaults.coeff[0][0][0][0] : probs_before;
  if ( key ) {
    aa::EstKeyCosts C;
    aa::enc_fill_key_costs( C.enc, quant[1] );
    C.full_mbw = fmbw; C.full_mbh = fmbh;
    J.costs = &C;
    if ( fill ) walk<FilledKeyPolicy>( J, nmb ); else walk<aa::EstimateKeyPolicy>( J, nmb );
  } else {
    aa::EstInterCosts C;
    uint8_t probs[2][19];
    std::memcpy( probs, probs_before + 1063, 38 );
    aa::enc_fill_inter_costs( C.enc, probs, quality, quant[1], static_cast<unsigned>( q_index ) );
    if ( !carry[3] ) { std::memset( C.enc.base.mv_comp, 0, sizeof C.enc.base.mv_comp ); std::memset( C.enc.mv_sad, 0, sizeof C.enc.mv_sad ); }
    C.full_mbw = fmbw; C.full_mbh = fmbh;
    J.costs = &C;
    if ( fill ) walk<FilledInterPolicy>( J, nmb ); else walk<aa::EstimateInterPolicy>( J, nmb );
  }
  g_fill = 0;
  aa::BoolWriter w0;
  const aa::est::Counts c = aa::est::write_tokens( w0, token_probs, mbs.data(), masks.data(), dense.data(), mbw, mbh );
  const size_t bytes = aa::estimate_frame_bytes( key != 0, static_cast<uint16_t>( w / 4 ), static_cast<uint16_t>( h / 4 ), static_cast<uint8_t>( q_index ), probs_before, mbs.data(),
                                                 masks.data(), c.token_bytes, c.with_coefficients, c.intra, carry );
  if ( size ) *size = uint64_t( bytes ) * 16;
  for ( size_t mi = 0; mi < nmb; mi++ )
    for ( int b = 0; b < 25; b++ ) if ( !( ( masks[mi] >> b ) & 1u ) ) std::memset( dense.data() + ( mi * 25 + b ) * 16, 0, 32 );
  if ( mbs_out ) std::memcpy( mbs_out, mbs.data(), nmb * sizeof( aa_mb_info ) );
  if ( dense_out ) std::memcpy( dense_out, dense.data(), nmb * 800 );
  return 0;
}

// The search of encode_with_target_size over estimate_sim: quants[q] are the factors of index q (128 x 6).  visited_q / visited_size: room
// for 8.  -> the chosen index, *steps estimates; the carry runs through the visited candidates.
int estimate_sim_target( int key, int w, int h, const uint8_t * ref, const uint8_t * target, const uint16_t * quants, int quality, const uint8_t * probs_before, uint8_t carry[4],
                         int fill, int q_lo, int q_hi, uint64_t target_size, int * steps, int * visited_q, uint64_t * visited_size )
{
  aa::QiChoice c;
  aa::qi_choice_begin( c, q_lo, q_hi );
  while ( !aa::qi_choice_done( c ) ) {
    if ( c.steps >= 8 ) return -1;
    const int q = aa::qi_choice_candidate( c );
    uint64_t size = 0;
    if ( estimate_sim( key, w, h, ref, target, q, quants + q * 6, quality, probs_before, carry, fill, &size, nullptr, nullptr ) ) return -1;
    visited_q[c.steps] = q; visited_size[c.steps] = size;
    aa::qi_choice_step( c, size, target_size );
  }
  *steps = c.steps;
  return c.best;
}

} // extern "C"

#if defined( ESTIMATE_SIM_MAIN )
// case file: int32 key, w, h, quality, q_index, fill; uint16 quant[6]; uint8 carry[4]; uint8 probs_before[1101]; uint8 pad[3]; ref planes
// (absent for a key estimate); target planes; then uint64 the reference's estimate (0: not compared)
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
    const size_t head = 24 + 12 + 4 + 1101 + 3;
    if ( d.size() < head ) { std::fprintf( stderr, "%s: short file\n", argv[a] ); return 2; }
    int32_t h[6]; uint16_t quant[6]; uint8_t carry[4];
    std::memcpy( h, d.data(), 24 ); std::memcpy( quant, d.data() + 24, 12 ); std::memcpy( carry, d.data() + 36, 4 );
    std::vector<uint8_t> probs( d.begin() + 40, d.begin() + 40 + 1101 );
    if ( h[1] < 4 || h[2] < 4 ) { std::fprintf( stderr, "%s: not a case file\n", argv[a] ); return 2; }
    const size_t planes = size_t( ( h[1] + 15 ) / 16 ) * ( ( h[2] + 15 ) / 16 ) * 384;
    if ( d.size() != head + ( h[0] ? 1 : 2 ) * planes + 8 ) { std::fprintf( stderr, "%s: not a case file\n", argv[a] ); return 2; }
    // (copies of their own: a read beyond a plane is a read beyond an allocation)
    std::vector<uint8_t> ref( h[0] ? d.begin() + head : d.begin() + head, d.begin() + head + ( h[0] ? 0 : planes ) );
    std::vector<uint8_t> target( d.begin() + head + ( h[0] ? 0 : planes ), d.begin() + head + ( h[0] ? 1 : 2 ) * planes );
    uint64_t want = 0, got = 0;
    std::memcpy( &want, d.data() + d.size() - 8, 8 );
    if ( estimate_sim( h[0], h[1], h[2], h[0] ? nullptr : ref.data(), target.data(), h[4], quant, h[3], probs.data(), carry, h[5], &got, nullptr, nullptr ) ) return 2;
    const bool same = !want || want == got;
    std::printf( "%s: estimate %llu%s\n", argv[a], static_cast<unsigned long long>( got ), same ? "" : " DIFFERS from the reference" );
    bad += !same;
  }
  return bad ? 1 : 0;
}
#endif
