// The per-block device functions of the rebase and the re-encode (rebase_kernels.hip, reencode_kernels.hip): the prediction of a 4x4
// unit, the forward path (subtract, DCT, division), the decoder's way back, the Y2 block, a chroma block, and the LDS picture of an
// intra macroblock's neighbourhood.  One source for both files; marked AA_MHD so that tests/cpp/reencode_sim.cc runs the same
// statements on the host.  The arithmetic itself is vp8_math.hh's.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "device_types.h"
#include "parse_common.hh"      // the mode enums
#include "vp8_math.hh"

namespace aa {
namespace {

constexpr int kLanes = 64;
enum : int { Q_Y_DC, Q_Y_AC, Q_Y2_DC, Q_Y2_AC, Q_UV_DC, Q_UV_AC };

AA_MHD int clampi( int v, int lo, int hi ) { return v < lo ? lo : ( v > hi ? hi : v ); }

// The decoder's inter prediction of one 4x4 unit at (x0, y0) of a w x h plane (prediction.cc:813-971): a 9x9 window around the
// vector's whole-pel position, coordinates clamped at the plane edges, horizontal then vertical six taps with the u8 clamp between
// (fraction 0: the taps {0,0,128,0,0,0}, which sixtap() turns into a copy).  p[row * 4 + col].
AA_MHD void predict_unit( const uint8_t * plane, const int w, const int h, const int x0, const int y0, const int mvx, const int mvy, int ( &p )[16] )
{
  const int fx = mvx & 7, fy = mvy & 7;
  const int sx = x0 + ( mvx >> 3 ) - 2, sy = y0 + ( mvy >> 3 ) - 2;
  int hx[6], vy[6];
#pragma unroll
  for ( int i = 0; i < 6; i++ ) { hx[i] = sixtap_coeff( fx, i ); vy[i] = sixtap_coeff( fy, i ); }
  int xs[9];
#pragma unroll
  for ( int c = 0; c < 9; c++ ) xs[c] = clampi( sx + c, 0, w - 1 );
  int t[9][4];
#pragma unroll
  for ( int r = 0; r < 9; r++ ) {
    const uint8_t * line = plane + static_cast<size_t>( clampi( sy + r, 0, h - 1 ) ) * w;
    int s[9];
#pragma unroll
    for ( int c = 0; c < 9; c++ ) s[c] = line[xs[c]];
#pragma unroll
    for ( int c = 0; c < 4; c++ ) t[r][c] = sixtap( s[c], s[c + 1], s[c + 2], s[c + 3], s[c + 4], s[c + 5], hx[0], hx[1], hx[2], hx[3], hx[4], hx[5] );
  }
#pragma unroll
  for ( int r = 0; r < 4; r++ )
#pragma unroll
    for ( int c = 0; c < 4; c++ ) p[r * 4 + c] = sixtap( t[r][c], t[r + 1][c], t[r + 2][c], t[r + 3][c], t[r + 4][c], t[r + 5][c], vy[0], vy[1], vy[2], vy[3], vy[4], vy[5] );
}

// target - prediction -> the 16 coefficients of the block, raster order (DCTCoefficients::subtract_dct)
AA_MHD void forward_block( const uint8_t * target, const int64_t stride, const int ( &p )[16], int ( &c )[16] )
{
  int im[16];
#pragma unroll
  for ( int r = 0; r < 4; r++ ) {
    const uint8_t * line = target + r * stride;
    const Quad v = fdct_pass1( line[0] - p[r * 4], line[1] - p[r * 4 + 1], line[2] - p[r * 4 + 2], line[3] - p[r * 4 + 3] );
    im[r * 4] = v.v0; im[r * 4 + 1] = v.v1; im[r * 4 + 2] = v.v2; im[r * 4 + 3] = v.v3;
  }
#pragma unroll
  for ( int i = 0; i < 4; i++ ) {
    const Quad v = fdct_pass2( im[i], im[i + 4], im[i + 8], im[i + 12] );
    c[i] = v.v0; c[i + 4] = v.v1; c[i + 8] = v.v2; c[i + 12] = v.v3;
  }
}

// c := c / factors in place; -> whether a coefficient is left
AA_MHD bool quantize_block( int ( &c )[16], const int fdc, const int fac )
{
  int any = 0;
#pragma unroll
  for ( int i = 0; i < 16; i++ ) { c[i] = quantize( c[i], i == 0 ? fdc : fac ); any |= c[i]; }
  return any != 0;
}

AA_MHD void store_block( int16_t * dst, const int ( &q )[16] )
{
#if defined( __HIPCC__ )
  uint32_t d[8];
#pragma unroll
  for ( int i = 0; i < 8; i++ ) d[i] = ( static_cast<uint32_t>( q[2 * i] ) & 0xFFFFu ) | ( static_cast<uint32_t>( q[2 * i + 1] ) << 16 );
  uint4 * o = reinterpret_cast<uint4 *>( dst );
  o[0] = make_uint4( d[0], d[1], d[2], d[3] ); o[1] = make_uint4( d[4], d[5], d[6], d[7] );
#else
  for ( int i = 0; i < 16; i++ ) dst[i] = static_cast<int16_t>( q[i] );
#endif
}

// the decoder's side of a block: dequantise (int16 wrap, Q4), the block's DC from the iWHT where a Y2 block is coded, IDCT (Q5);
// -> the four rows of prediction + residual as packed pixels
AA_MHD void reconstruct_block( const int ( &q )[16], const int fdc, const int fac, const bool replace_dc, const int dc, const int ( &p )[16], uint32_t ( &rows )[4] )
{
  int c[16], im[16];
#pragma unroll
  for ( int i = 0; i < 16; i++ ) c[i] = dequant( q[i], i == 0 ? fdc : fac );
  if ( replace_dc ) c[0] = dc;
#pragma unroll
  for ( int i = 0; i < 4; i++ ) { const Quad v = idct_pass1( c[i], c[i + 4], c[i + 8], c[i + 12] ); im[i * 4] = v.v0; im[i * 4 + 1] = v.v1; im[i * 4 + 2] = v.v2; im[i * 4 + 3] = v.v3; }
#pragma unroll
  for ( int i = 0; i < 4; i++ ) {
    const Quad v = idct_pass2( im[i], im[i + 4], im[i + 8], im[i + 12] );
    rows[i] = static_cast<uint32_t>( clamp255( p[i * 4] + v.v0 ) ) | ( static_cast<uint32_t>( clamp255( p[i * 4 + 1] + v.v1 ) ) << 8 )
              | ( static_cast<uint32_t>( clamp255( p[i * 4 + 2] + v.v2 ) ) << 16 ) | ( static_cast<uint32_t>( clamp255( p[i * 4 + 3] + v.v3 ) ) << 24 );
  }
}

// The Y2 block of a macroblock from its 16 luma DCs (raster order, in LDS): forward WHT, division by the Y2 factors -> q2; then the
// decoder's way back -- dequantise, inverse WHT -- to the DC luma block b is reconstructed with.  Every lane of the macroblock
// computes the whole block (16 values); -> whether q2 holds a coefficient.
AA_MHD bool y2_block( const int16_t * dcs, const uint16_t * quant, const int b, int ( &q2 )[16], int & dc_back )
{
  int w1[16];
#pragma unroll
  for ( int i = 0; i < 4; i++ ) { const Quad v = fwht_pass1( dcs[4 * i], dcs[4 * i + 1], dcs[4 * i + 2], dcs[4 * i + 3] ); w1[4 * i] = v.v0; w1[4 * i + 1] = v.v1; w1[4 * i + 2] = v.v2; w1[4 * i + 3] = v.v3; }
#pragma unroll
  for ( int i = 0; i < 4; i++ ) { const Quad v = fwht_pass2( w1[i], w1[i + 4], w1[i + 8], w1[i + 12] ); q2[i] = v.v0; q2[i + 4] = v.v1; q2[i + 8] = v.v2; q2[i + 12] = v.v3; }
  const bool any = quantize_block( q2, quant[Q_Y2_DC], quant[Q_Y2_AC] );
  int c[16], im[16];
#pragma unroll
  for ( int i = 0; i < 16; i++ ) c[i] = dequant( q2[i], i == 0 ? quant[Q_Y2_DC] : quant[Q_Y2_AC] );
#pragma unroll
  for ( int i = 0; i < 4; i++ ) { const Quad v = iwht_pass1( c[i], c[i + 4], c[i + 8], c[i + 12] ); im[i] = v.v0; im[i + 4] = v.v1; im[i + 8] = v.v2; im[i + 12] = v.v3; }
  dc_back = 0;
#pragma unroll
  for ( int i = 0; i < 4; i++ ) {
    const Quad v = iwht_pass2( im[4 * i], im[4 * i + 1], im[4 * i + 2], im[4 * i + 3] );
    dc_back = b == 4 * i ? v.v0 : dc_back; dc_back = b == 4 * i + 1 ? v.v1 : dc_back;
    dc_back = b == 4 * i + 2 ? v.v2 : dc_back; dc_back = b == 4 * i + 3 ? v.v3 : dc_back;
  }
  dc_back = static_cast<int16_t>( dc_back );
  return any;
}

AA_MHD void store_rows( uint8_t * dst, const int stride, const uint32_t ( &rows )[4] )
{
#pragma unroll
  for ( int r = 0; r < 4; r++ ) *reinterpret_cast<uint32_t *>( dst + static_cast<size_t>( r ) * stride ) = rows[r];
}

// One chroma block (cb: 0..3 of plane pl) with its prediction in p: forward path, its slot, its reconstruction; -> non-zero
AA_MHD bool chroma_block( const aa_rebase_dev_job & J, const size_t mi, const int col, const int row, const int pl, const int cb, const int ( &p )[16] )
{
  const int cw = J.mbw * 8;
  const int x0 = col * 8 + ( cb & 1 ) * 4, y0 = row * 8 + ( cb >> 1 ) * 4;
  int q[16];
  forward_block( J.target[1 + pl] + static_cast<int64_t>( y0 ) * J.target_stride[1] + x0, J.target_stride[1], p, q );
  const bool nz = quantize_block( q, J.quant[Q_UV_DC], J.quant[Q_UV_AC] );
  store_block( J.coeffs + ( mi * 25 + 16 + pl * 4 + cb ) * 16, q );
  if ( J.has_intra ) {
    uint32_t rows[4];
    reconstruct_block( q, J.quant[Q_UV_DC], J.quant[Q_UV_AC], false, 0, p, rows );
    store_rows( J.recon[1 + pl] + static_cast<size_t>( y0 ) * cw + x0, cw, rows );
  }
  return nz;
}

struct alignas( 16 ) RebaseIntraLds {
  alignas( 16 ) uint8_t y[17][24];    // [row+1][col+4]: row -1 = above (cols -4..19 incl. above-right), col -1 = left; B_PRED: filled in as sub-blocks are reconstructed
  alignas( 16 ) uint8_t c[2][9][12];  // chroma: [plane][row+1][col+4]
  alignas( 16 ) uint8_t edge[16];     // B_PRED: E[0..12] of the current sub-block (vp8_math.hh bpred_pixel)
  alignas( 16 ) uint8_t pred[16];     // ... and its prediction
  alignas( 16 ) int16_t dcs[16];
};

// pixels of the new frame's reconstruction that this launch -- this very wave -- may have stored: read past the CU's L1
AA_MHD uint32_t load_recon_u32( const uint8_t * p )
{
#if defined( __HIP_DEVICE_COMPILE__ )
  return __hip_atomic_load( reinterpret_cast<const uint32_t *>( p ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
#else
  return *reinterpret_cast<const uint32_t *>( p );
#endif
}

} // namespace
} // namespace aa
