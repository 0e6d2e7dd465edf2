// The rebase (aa_rebase_batch; Encoder::update_residues / update_macroblock, reencode.cc:131-303): every prediction mode and motion
// vector of an inter frame is kept and its residues are recomputed against the job stream's CURRENT references -- predict, subtract
// the prediction from the target, forward DCT (forward WHT of the 16 luma DCs where a Y2 block is coded), quantise by plain division,
// reconstruct.  Batched: blockIdx.y is the job (one stream's new frame), jobs are independent.
//
//   k_rebase_inter   every inter-coded macroblock of every job.  16 lanes per macroblock, four macroblocks per wave; lane b owns luma
//                    block b (lanes 0..7 also one chroma block each).  A lane predicts its 4x4 unit with the decoder's six taps from a
//                    9x9 window it reads with coordinate clamping (whole-vector and SPLITMV macroblocks are the same code: a 16x16
//                    prediction is its sixteen 4x4 units), runs the forward path in registers and stores its slot of the dense
//                    scratch; the 16 DCs meet in LDS for the WHT.  No atomics, no workgroup talks to another.
//   k_rebase_intra   the intra macroblocks of a job, in raster order, by ONE wave per job: their prediction reads unfiltered
//                    reconstructed neighbours of the new frame -- inter macroblocks (all written by the first kernel) or intra ones
//                    earlier in raster order -- so a single wave walking the frame needs no hand-off between workgroups.  Frames that
//                    are mostly intra run slowly here.
//
// The arithmetic is vp8_math.hh's (fdct_pass1/2, fwht_pass1/2, quantize, and the decoder's own dequant / idct / iwht / sixtap /
// predictors), so host and device compile one source (tests/cpp/forward_math_check.cc).
#include <hip/hip_runtime.h>
#include <algorithm>

#include "device_types.h"
#include "vp8_math.hh"

namespace aa {
namespace {

constexpr int kLanes = 64;
enum : int { DC_PRED, V_PRED, H_PRED, TM_PRED, B_PRED, NEARESTMV, NEARMV, ZEROMV, NEWMV, SPLITMV };
enum : int { Q_Y_DC, Q_Y_AC, Q_Y2_DC, Q_Y2_AC, Q_UV_DC, Q_UV_AC };

__device__ __forceinline__ int clampi( int v, int lo, int hi ) { return v < lo ? lo : ( v > hi ? hi : v ); }

// The decoder's inter prediction of one 4x4 unit at (x0, y0) of a w x h plane (prediction.cc:813-971): a 9x9 window around the
// vector's whole-pel position, coordinates clamped at the plane edges, horizontal then vertical six taps with the u8 clamp between
// (fraction 0: the taps {0,0,128,0,0,0}, which sixtap() turns into a copy).  p[row * 4 + col].
__device__ __forceinline__ void predict_unit( const uint8_t * plane, const int w, const int h, const int x0, const int y0, const int mvx, const int mvy, int ( &p )[16] )
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
__device__ __forceinline__ void forward_block( const uint8_t * target, const int64_t stride, const int ( &p )[16], int ( &c )[16] )
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
__device__ __forceinline__ bool quantize_block( int ( &c )[16], const int fdc, const int fac )
{
  int any = 0;
#pragma unroll
  for ( int i = 0; i < 16; i++ ) { c[i] = quantize( c[i], i == 0 ? fdc : fac ); any |= c[i]; }
  return any != 0;
}

__device__ __forceinline__ void store_block( int16_t * dst, const int ( &q )[16] )
{
  uint32_t d[8];
#pragma unroll
  for ( int i = 0; i < 8; i++ ) d[i] = ( static_cast<uint32_t>( q[2 * i] ) & 0xFFFFu ) | ( static_cast<uint32_t>( q[2 * i + 1] ) << 16 );
  uint4 * o = reinterpret_cast<uint4 *>( dst );
  o[0] = make_uint4( d[0], d[1], d[2], d[3] ); o[1] = make_uint4( d[4], d[5], d[6], d[7] );
}

// the decoder's side of a block: dequantise (int16 wrap, Q4), the block's DC from the iWHT where a Y2 block is coded, IDCT (Q5);
// -> the four rows of prediction + residual as packed pixels
__device__ __forceinline__ void reconstruct_block( const int ( &q )[16], const int fdc, const int fac, const bool replace_dc, const int dc, const int ( &p )[16], uint32_t ( &rows )[4] )
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
__device__ __forceinline__ bool y2_block( const int16_t * dcs, const uint16_t * quant, const int b, int ( &q2 )[16], int & dc_back )
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

__device__ __forceinline__ void store_rows( uint8_t * dst, const int stride, const uint32_t ( &rows )[4] )
{
#pragma unroll
  for ( int r = 0; r < 4; r++ ) *reinterpret_cast<uint32_t *>( dst + static_cast<size_t>( r ) * stride ) = rows[r];
}

// One chroma block (cb: 0..3 of plane pl) with its prediction in p: forward path, its slot, its reconstruction; -> non-zero
__device__ __forceinline__ bool chroma_block( const aa_rebase_dev_job & J, const size_t mi, const int col, const int row, const int pl, const int cb, const int ( &p )[16] )
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

} // namespace

// grid.x = quad of macroblocks, grid.y = job
__global__ __launch_bounds__( kLanes ) void k_rebase_inter( const aa_rebase_dev_job * jobs )
{
  __shared__ int16_t dcs[4][16];
  const aa_rebase_dev_job & J = jobs[blockIdx.y];
  const unsigned total = static_cast<unsigned>( J.mbw ) * J.mbh;
  if ( blockIdx.x * 4u >= total ) return;                   // (whole workgroup: jobs of one call may differ in size)
  const int slot = threadIdx.x >> 4, b = threadIdx.x & 15;
  const unsigned want = blockIdx.x * 4u + slot;
  const size_t mi = want < total ? want : total - 1;        // lanes without a macroblock of their own run along on the last one and store nothing
  const aa_mb_info & mb = J.mbs[mi];
  const bool active = want < total && mb.ref_frame != 0;
  const int col = static_cast<int>( mi % J.mbw ), row = static_cast<int>( mi / J.mbw );
  const int pw = J.mbw * 16, ph = J.mbh * 16, cw = pw >> 1, ch = ph >> 1;
  const uint8_t * const * ref = J.ref[mb.ref_frame ? ( mb.ref_frame & 3 ) : 1];
  const bool has_y2 = mb.y_mode != SPLITMV;

  // ---- luma block b ----
  const int x0 = col * 16 + ( b & 3 ) * 4, y0 = row * 16 + ( b >> 2 ) * 4;
  int p[16], q[16];
  predict_unit( ref[0], pw, ph, x0, y0, mb.u.mv[b][0], mb.u.mv[b][1], p );
  forward_block( J.target[0] + static_cast<int64_t>( y0 ) * J.target_stride[0] + x0, J.target_stride[0], p, q );
  dcs[slot][b] = static_cast<int16_t>( q[0] );
  if ( has_y2 ) q[0] = 0;
  const bool nz = quantize_block( q, J.quant[Q_Y_DC], J.quant[Q_Y_AC] );
  if ( active ) store_block( J.coeffs + ( mi * 25 + b ) * 16, q );
  __syncthreads();
  int q2[16], dc_back = 0;
  bool nz2 = false;
  if ( has_y2 ) {
    nz2 = y2_block( dcs[slot], J.quant, b, q2, dc_back );
    if ( active && b == 0 ) store_block( J.coeffs + ( mi * 25 + 24 ) * 16, q2 );
  }
  if ( active && J.has_intra ) {
    uint32_t rows[4];
    reconstruct_block( q, J.quant[Q_Y_DC], J.quant[Q_Y_AC], has_y2, dc_back, p, rows );
    store_rows( J.recon[0] + static_cast<size_t>( y0 ) * pw + x0, pw, rows );
  }

  // ---- chroma: lanes 0..7 one block each, with the rounded average of the four luma vectors above it ----
  bool nzc = false;
  if ( b < 8 ) {
    const int pl = b >> 2, cb = b & 3, i0 = ( cb >> 1 ) * 8 + ( cb & 1 ) * 2;
    const int mvx = chroma_mv( mb.u.mv[i0][0] + mb.u.mv[i0 + 1][0] + mb.u.mv[i0 + 4][0] + mb.u.mv[i0 + 5][0] );
    const int mvy = chroma_mv( mb.u.mv[i0][1] + mb.u.mv[i0 + 1][1] + mb.u.mv[i0 + 4][1] + mb.u.mv[i0 + 5][1] );
    predict_unit( ref[1 + pl], cw, ch, col * 8 + ( cb & 1 ) * 4, row * 8 + ( cb >> 1 ) * 4, mvx, mvy, p );
    if ( active ) nzc = chroma_block( J, mi, col, row, pl, cb, p );
  }
  const unsigned long long by = __ballot( nz ), bc = __ballot( nzc );
  if ( active && b == 0 )
    J.masks[mi] = static_cast<uint32_t>( ( by >> ( slot * 16 ) ) & 0xFFFFu ) | ( static_cast<uint32_t>( ( bc >> ( slot * 16 ) ) & 0xFFu ) << 16 ) | ( nz2 ? 1u << 24 : 0u );
}

namespace {

struct alignas( 16 ) RebaseIntraLds {
  alignas( 16 ) uint8_t y[17][24];    // [row+1][col+4]: row -1 = above (cols -4..19 incl. above-right), col -1 = left; B_PRED: filled in as sub-blocks are reconstructed
  alignas( 16 ) uint8_t c[2][9][12];  // chroma: [plane][row+1][col+4]
  alignas( 16 ) uint8_t edge[16];     // B_PRED: E[0..12] of the current sub-block (vp8_math.hh bpred_pixel)
  alignas( 16 ) uint8_t pred[16];     // ... and its prediction
  alignas( 16 ) int16_t dcs[16];
};

// pixels of the new frame's reconstruction that this launch -- this very wave -- may have stored: read past the CU's L1
__device__ __forceinline__ uint32_t load_recon_u32( const uint8_t * p )
{
  return __hip_atomic_load( reinterpret_cast<const uint32_t *>( p ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
}

// One intra macroblock by the whole wave: Encoder::update_macroblock's intra branches (reencode.cc:144-166,217-233) with the key-frame
// edge rules of VP8Raster::Block<N>::predictors (prediction.cc:99-167), laid out as the decoder's intra_macroblock (kernels.hip).
__device__ void rebase_intra_macroblock( const aa_rebase_dev_job & J, const size_t mi, RebaseIntraLds & L, const int lane )
{
  const aa_mb_info & mb = J.mbs[mi];
  const int col = static_cast<int>( mi % J.mbw ), row = static_cast<int>( mi / J.mbw );
  const int pw = J.mbw * 16, cw = pw >> 1;
  const int x0 = col * 16, y0 = row * 16;
  const uint8_t * Y = J.recon[0];
  if ( lane < 6 ) {
    uint32_t v;
    if ( y0 == 0 ) v = 0x7F7F7F7Fu;
    else if ( lane == 0 ) v = x0 > 0 ? load_recon_u32( Y + static_cast<size_t>( y0 - 1 ) * pw + x0 - 4 ) : 0x81818181u;
    else if ( lane <= 4 ) v = load_recon_u32( Y + static_cast<size_t>( y0 - 1 ) * pw + x0 + ( lane - 1 ) * 4 );
    else if ( x0 + 16 >= pw ) v = 0x01010101u * ( load_recon_u32( Y + static_cast<size_t>( y0 - 1 ) * pw + pw - 4 ) >> 24 );   // replicate: prediction.cc:144-151
    else v = load_recon_u32( Y + static_cast<size_t>( y0 - 1 ) * pw + x0 + 16 );
    *reinterpret_cast<uint32_t *>( &L.y[0][lane * 4] ) = v;
  } else if ( lane >= 32 && lane < 48 ) {
    const int r = lane - 32;
    L.y[r + 1][3] = x0 > 0 ? static_cast<uint8_t>( load_recon_u32( Y + static_cast<size_t>( y0 + r ) * pw + x0 - 4 ) >> 24 ) : 129;
  }
  {
    const int cx0 = col * 8, cy0 = row * 8;
    const int pl = lane >> 5, l = lane & 31;
    const uint8_t * C = J.recon[1 + pl];
    if ( l < 3 ) {
      uint32_t v;
      if ( cy0 == 0 ) v = 0x7F7F7F7Fu;
      else if ( l == 0 ) v = cx0 > 0 ? load_recon_u32( C + static_cast<size_t>( cy0 - 1 ) * cw + cx0 - 4 ) : 0x81818181u;
      else v = load_recon_u32( C + static_cast<size_t>( cy0 - 1 ) * cw + cx0 + ( l - 1 ) * 4 );
      *reinterpret_cast<uint32_t *>( &L.c[pl][0][l * 4] ) = v;
    } else if ( l >= 16 && l < 24 ) {
      const int r = l - 16;
      L.c[pl][r + 1][3] = cx0 > 0 ? static_cast<uint8_t>( load_recon_u32( C + static_cast<size_t>( cy0 + r ) * cw + cx0 - 4 ) >> 24 ) : 129;
    }
  }
  __syncthreads();

  // ---- chroma, lanes 16..23: U then V, 8x8 prediction with uv_mode, block by block ----
  bool nz = false;
  if ( lane >= 16 && lane < 24 ) {
    const int pl = ( lane - 16 ) >> 2, cb = lane & 3;
    int sa = 0, sl = 0;
    for ( int i = 0; i < 8; i++ ) { sa += L.c[pl][0][i + 4]; sl += L.c[pl][i + 1][3]; }
    const int dc = bigpred_dc( sa, sl, row > 0, col > 0, 3 ), corner = L.c[pl][0][3];
    int p[16];
#pragma unroll
    for ( int r = 0; r < 4; r++ )
#pragma unroll
      for ( int c = 0; c < 4; c++ ) p[r * 4 + c] = bigpred_pixel( mb.uv_mode, L.c[pl][0][( cb & 1 ) * 4 + c + 4], L.c[pl][( cb >> 1 ) * 4 + r + 1][3], corner, dc );
    nz = chroma_block( J, mi, col, row, pl, cb, p );
  }

  if ( mb.y_mode != B_PRED ) {
    // ---- 16x16: lanes 0..15 one luma block each, Y2 as for non-split inter (encode_intra.cc:169-222, FIRST_PASS) ----
    int p[16], q[16];
    const int b = lane & 15, bx = ( b & 3 ) * 4, by = ( b >> 2 ) * 4;
    if ( lane < 16 ) {
      int sa = 0, sl = 0;
      for ( int i = 0; i < 16; i++ ) { sa += L.y[0][i + 4]; sl += L.y[i + 1][3]; }
      const int dc = bigpred_dc( sa, sl, row > 0, col > 0, 4 ), corner = L.y[0][3];
#pragma unroll
      for ( int r = 0; r < 4; r++ )
#pragma unroll
        for ( int c = 0; c < 4; c++ ) p[r * 4 + c] = bigpred_pixel( mb.y_mode, L.y[0][bx + c + 4], L.y[by + r + 1][3], corner, dc );
      forward_block( J.target[0] + static_cast<int64_t>( y0 + by ) * J.target_stride[0] + x0 + bx, J.target_stride[0], p, q );
      L.dcs[b] = static_cast<int16_t>( q[0] );
      q[0] = 0;
      nz = quantize_block( q, J.quant[Q_Y_DC], J.quant[Q_Y_AC] );
      store_block( J.coeffs + ( mi * 25 + b ) * 16, q );
    }
    __syncthreads();
    bool nz2 = false;
    if ( lane < 16 ) {
      int q2[16], dc_back;
      nz2 = y2_block( L.dcs, J.quant, b, q2, dc_back );
      if ( lane == 0 ) store_block( J.coeffs + ( mi * 25 + 24 ) * 16, q2 );
      uint32_t rows[4];
      reconstruct_block( q, J.quant[Q_Y_DC], J.quant[Q_Y_AC], true, dc_back, p, rows );
      store_rows( J.recon[0] + static_cast<size_t>( y0 + by ) * pw + x0 + bx, pw, rows );
    }
    const unsigned long long m = __ballot( nz );
    if ( lane == 0 ) J.masks[mi] = static_cast<uint32_t>( m & 0xFFFFFFu ) | ( nz2 ? 1u << 24 : 0u );
  } else {
    // ---- B_PRED: sub-block by sub-block in raster order, each reconstructed before the next one predicts (encode_intra.cc:48-71) ----
    const unsigned long long mc = __ballot( nz );
    uint32_t ymask = 0;
    for ( int sb = 0; sb < 16; sb++ ) {
      const int bx = sb & 3, by = sb >> 2;
      const int ar = by * 4, ac = bx * 4 + 3;       // LDS index of (row -1, col -1) of this sub-block
      if ( lane < 13 ) {
        uint8_t e;
        if ( lane < 4 ) e = L.y[ar + 4 - lane][ac];
        else if ( lane < 9 ) e = L.y[ar][ac + lane - 4];
        else e = bx == 3 ? L.y[0][20 + lane - 9] : L.y[ar][ac + lane - 4];   // above-right of the fourth column: the row above the MACROBLOCK (prediction.cc:140-164)
        L.edge[lane] = e;
      }
      __syncthreads();
      if ( lane < 16 ) L.pred[lane] = static_cast<uint8_t>( bpred_pixel( mb.u.b_mode[sb], L.edge, lane & 3, lane >> 2 ) );
      __syncthreads();
      if ( lane == 0 ) {
        int p[16], q[16];
#pragma unroll
        for ( int i = 0; i < 16; i++ ) p[i] = L.pred[i];
        forward_block( J.target[0] + static_cast<int64_t>( y0 + by * 4 ) * J.target_stride[0] + x0 + bx * 4, J.target_stride[0], p, q );
        if ( quantize_block( q, J.quant[Q_Y_DC], J.quant[Q_Y_AC] ) ) ymask |= 1u << sb;
        store_block( J.coeffs + ( mi * 25 + sb ) * 16, q );
        uint32_t rows[4];
        reconstruct_block( q, J.quant[Q_Y_DC], J.quant[Q_Y_AC], false, 0, p, rows );
#pragma unroll
        for ( int r = 0; r < 4; r++ ) *reinterpret_cast<uint32_t *>( &L.y[ar + r + 1][bx * 4 + 4] ) = rows[r];
      }
      __syncthreads();
    }
    {
      const int r = lane >> 2, c4 = ( lane & 3 ) * 4;
      *reinterpret_cast<uint32_t *>( J.recon[0] + static_cast<size_t>( y0 + r ) * pw + x0 + c4 ) = *reinterpret_cast<const uint32_t *>( &L.y[r + 1][c4 + 4] );
    }
    if ( lane == 0 ) J.masks[mi] = ymask | static_cast<uint32_t>( mc & 0xFF0000u );
  }
  __threadfence();        // the next intra macroblock of this wave reads these pixels back from memory
  __syncthreads();
}

} // namespace

// grid.x = 1, grid.y = job: one wave walks the job's records 64 at a time and takes the intra macroblocks in raster order
__global__ __launch_bounds__( kLanes ) void k_rebase_intra( const aa_rebase_dev_job * jobs )
{
  __shared__ RebaseIntraLds L;
  const aa_rebase_dev_job & J = jobs[blockIdx.y];
  if ( !J.has_intra ) return;
  const int lane = threadIdx.x;
  const unsigned total = static_cast<unsigned>( J.mbw ) * J.mbh;
  for ( unsigned base = 0; base < total; base += kLanes ) {
    const unsigned mi = base + lane;
    unsigned long long intra = __ballot( mi < total && J.mbs[mi < total ? mi : 0].ref_frame == 0 );
    while ( intra ) {
      const int k = __ffsll( static_cast<long long>( intra ) ) - 1;
      intra &= intra - 1;
      rebase_intra_macroblock( J, base + k, L, lane );
    }
  }
}

int launch_rebase( const aa_rebase_dev_job * jobs, int n, uint32_t max_mbs, bool any_intra, void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  for ( int base = 0; base < n; base += 32768 ) {
    const int cnt = std::min( 32768, n - base );
    hipLaunchKernelGGL( k_rebase_inter, dim3( ( max_mbs + 3 ) / 4, cnt ), dim3( kLanes ), 0, st, jobs + base );
    if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
    if ( any_intra ) {
      hipLaunchKernelGGL( k_rebase_intra, dim3( 1, cnt ), dim3( kLanes ), 0, st, jobs + base );
      if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
    }
  }
  return 0;
}

} // namespace aa
