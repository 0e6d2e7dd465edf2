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
// The per-block device functions (predict_unit, forward_block, ..., chroma_block, the LDS picture) are rebase_inl.hh's, shared with the
// re-encode.  The arithmetic is vp8_math.hh's (fdct_pass1/2, fwht_pass1/2, quantize, and the decoder's own dequant / idct / iwht / sixtap /
// predictors), so host and device compile one source (tests/cpp/forward_math_check.cc).
#include <hip/hip_runtime.h>
#include <algorithm>

#include "device_types.h"
#include "rebase_inl.hh"
#include "vp8_math.hh"

namespace aa {

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
