// Test harness (not product code): the forward encoder's decision and forward path on the host, whole frames at a time.  It compiles the
// product's own headers -- reencode_search.hh (the three policies of the decision), reencode_mb.hh (one macroblock by sixteen lanes) and
// rebase_inl.hh (the per-block forward path) -- with `Lanes` = sixteen register files and a loop, under KeyPolicy and ForwardInterPolicy,
// and walks a frame's macroblocks in raster order where k_encode_key / k_encode_inter walk their anti-diagonals.  Built by
// tests/test_encode_sim.py with plain g++:
//   g++ -shared encode_sim.cc                              the library the test compares field by field
//   g++ -DENCODE_SIM_MAIN -fsanitize=... encode_sim.cc     a stand-alone program over case files: inputs, then what the reference wrote
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alfalfa_amd/csrc/reencode_mb.hh"

namespace {
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

// One frame.  key != 0: a key frame (ref and mv_probs unused, may be null).  ref / target: padded planes Y, U, V one after the other
// (stride = padded width); quant: {y_dc, y_ac, y2_dc, y2_ac, uv_dc, uv_ac}; q_index: the header's y_ac_qi; mv_probs: the stream's
// current [2][19]; quality: 0 best, 1 real-time.  Out: mbs (y_mode, uv_mode, ref_frame, nz_mask, u; the rest zero), dense [nmb][25][16]
// with zeros in every slot the mask leaves out, recon: the unfiltered reconstruction (planes as ref).
int encode_sim_frame( int key, int mbw, int mbh, const uint8_t * ref, const uint8_t * target, const uint16_t quant[6], int q_index, const uint8_t * mv_probs,
                      int quality, aa_mb_info * mbs, int16_t * dense, uint8_t * recon )
{
  const size_t nmb = size_t( mbw ) * mbh, ysz = nmb * 256, csz = nmb * 64;
  std::vector<uint32_t> masks( nmb, 0 ), nb( nmb * 4, 0 );
  aa_reencode_dev_job J;
  std::memset( &J, 0, sizeof J );
  if ( !key ) { J.base.ref[1][0] = ref; J.base.ref[1][1] = ref + ysz; J.base.ref[1][2] = ref + ysz + csz; }
  J.base.target[0] = target; J.base.target[1] = target + ysz; J.base.target[2] = target + ysz + csz;
  J.base.target_stride[0] = mbw * 16; J.base.target_stride[1] = mbw * 8;
  J.base.recon[0] = recon; J.base.recon[1] = recon + ysz; J.base.recon[2] = recon + ysz + csz;
  J.base.coeffs = dense; J.base.masks = masks.data();
  std::memcpy( J.base.quant, quant, sizeof J.base.quant );
  J.base.mbw = static_cast<uint16_t>( mbw ); J.base.mbh = static_cast<uint16_t>( mbh ); J.base.has_intra = 1;
  J.mbs_out = mbs; J.nb = nb.data();
  if ( key ) {
    aa::EncKeyCosts C;
    aa::enc_fill_key_costs( C, quant[1] );
    J.costs = &C;
    walk<aa::KeyPolicy>( J, nmb );
  } else {
    aa::EncInterCosts C;
    uint8_t probs[2][19];
    std::memcpy( probs, mv_probs, 38 );
    aa::enc_fill_inter_costs( C, probs, quality, quant[1], static_cast<unsigned>( q_index ) );
    J.costs = &C;
    walk<aa::ForwardInterPolicy>( J, nmb );
  }
  for ( size_t mi = 0; mi < nmb; mi++ )
    for ( int b = 0; b < 25; b++ ) if ( !( ( masks[mi] >> b ) & 1u ) ) std::memset( dense + ( mi * 25 + b ) * 16, 0, 32 );
  return 0;
}

// The host's side of a job's cost block, for the table test: update_rd_multipliers over a quantiser factor, the 256 SAD costs, the weight
void encode_sim_rd_multipliers( int y_ac, uint32_t out[2] ) { aa::enc_rd_multipliers( static_cast<uint16_t>( y_ac ), out[0], out[1] ); }
void encode_sim_mv_sad( uint16_t out[256] ) { uint16_t t[256]; aa::enc_fill_mv_sad( t ); std::memcpy( out, t, sizeof t ); }
int encode_sim_sad_per_bit( int q_index ) { return static_cast<int>( aa::enc_sad_per_bit( static_cast<unsigned>( q_index ) ) ); }
void encode_sim_prob_cost( uint16_t out[256] ) { std::memcpy( out, k_prob_cost, 512 ); }
void encode_sim_key_mode_costs( uint16_t out[5] ) { aa::EncKeyCosts C; aa::enc_fill_key_costs( C, 4 ); std::memcpy( out, C.mbmode, 10 ); }

} // extern "C"

#if defined( ENCODE_SIM_MAIN )
// case file: int32 key, mbw, mbh, quality, q_index; uint16 quant[6]; uint8 mv_probs[38]; ref planes (zeros for a key frame); target
// planes; then the reference's records [nmb] and dense coefficients [nmb][25][16]
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
    int32_t h[5]; uint16_t quant[6]; uint8_t probs[38];
    if ( d.size() < 70 ) { std::fprintf( stderr, "%s: short file\n", argv[a] ); return 2; }
    std::memcpy( h, d.data(), 20 ); std::memcpy( quant, d.data() + 20, 12 ); std::memcpy( probs, d.data() + 32, 38 );
    const size_t nmb = size_t( h[1] ) * h[2], planes = nmb * 384;
    if ( h[1] <= 0 || h[2] <= 0 || d.size() != 70 + 2 * planes + nmb * ( sizeof( aa_mb_info ) + 800 ) ) { std::fprintf( stderr, "%s: not a case file\n", argv[a] ); return 2; }
    const uint8_t * ref = d.data() + 70, * target = ref + planes;
    const uint8_t * want_mb = target + planes;
    const uint8_t * want_dense = want_mb + nmb * sizeof( aa_mb_info );
    std::vector<aa_mb_info> mbs( nmb );
    std::vector<int16_t> dense( nmb * 400 );
    std::vector<uint8_t> recon( planes );
    encode_sim_frame( h[0], h[1], h[2], ref, target, quant, h[4], probs, h[3], mbs.data(), dense.data(), recon.data() );
    size_t differ = 0;
    for ( size_t mi = 0; mi < nmb; mi++ ) {
      aa_mb_info w;
      std::memcpy( &w, want_mb + mi * sizeof w, sizeof w );
      const bool same = mbs[mi].y_mode == w.y_mode && mbs[mi].uv_mode == w.uv_mode && mbs[mi].ref_frame == w.ref_frame && mbs[mi].nz_mask == w.nz_mask
                        && !std::memcmp( &mbs[mi].u, &w.u, sizeof w.u ) && !std::memcmp( dense.data() + mi * 400, want_dense + mi * 800, 800 );
      if ( !same ) differ++;
    }
    std::printf( "%s: %zu of %zu macroblocks differ from the reference\n", argv[a], differ, nmb );
    bad += differ != 0;
  }
  return bad ? 1 : 0;
}
#endif
