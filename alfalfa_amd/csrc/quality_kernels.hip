// Quality of decoded frames against originals, batched and device-resident (aa_quality_batch_async): BaseRaster::quality
// (util/raster.cc:63-66 -> util/ssim.cc:57-71 -> libx264's pixel_ssim_wxh) and the sum of squared differences, per plane.
//
// The arithmetic is aa_ssim_host's (runtime_lf_search.inc), step for step: integer sums s1, s2, ss, s12 per 4x4 block, an 8x8
// window = 2x2 blocks (windows every 4 pixels), one window term in single precision (two multiplications, one correctly rounded
// division, nothing a contraction could fuse), terms added in x264's order -- four neighbouring terms left to right into a float,
// the groups one after another, row after row, into one float total -- then (double)total / (double)windows.  Every step is one
// correctly rounded IEEE operation in a fixed order, so the value is the host's bit for bit.
//
//   pass 1 (k_quality_blocks)  strips of block rows x (pair, plane): every pixel of both planes is read once (but for the block row
//                              two strips share), 16 bytes per lane and row, lanes along rows; block sums by v_dot4_u32_u8 on the
//                              packed bytes, kept in LDS; one float per group of four windows goes to HBM at its (row, group)
//                              place; the strip's squared differences (sum of ss - 2 s12 over its own blocks) are added to the
//                              plane's 64-bit word with one integer atomic per workgroup (integer addition: exact in any order).
//   pass 2 (k_quality_sum)     one wave per (pair, plane): the group values, which lie in x264's order, are staged in LDS by the
//                              whole wave and added up by one lane -- the chain is serial by definition.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_types.h"

namespace aa {
namespace {

constexpr int kStripRows = AA_QUALITY_STRIP_ROWS;      // window rows of a strip: kStripRows + 1 block rows are loaded
constexpr int kChunkWin = AA_QUALITY_CHUNK_WINDOWS;    // windows of a column chunk (wider planes are cut: the LDS is finite)
constexpr int kCols = kChunkWin + 4;                   // block columns a workgroup holds (the chunk's windows + 1, in whole 16-pixel tiles)
static_assert( kChunkWin % 4 == 0, "a chunk begins at a group of four windows and at a 16-pixel tile" );

// The planes and the workspace are HBM: pointers read from the job table are told so (global loads, not flat ones)
#define AA_GLOBAL __attribute__( ( address_space( 1 ) ) )
typedef uint32_t u32x4 __attribute__( ( ext_vector_type( 4 ) ) );
typedef float f32x4 __attribute__( ( ext_vector_type( 4 ) ) );
template <typename T> __device__ __forceinline__ const AA_GLOBAL T * in_hbm( const void * p ) { return reinterpret_cast<const AA_GLOBAL T *>( reinterpret_cast<uintptr_t>( p ) ); }

// four pixels of one row of one block; p is 4-byte aligned or read byte by byte
__device__ __forceinline__ uint32_t quad( const uint8_t * p )
{
  if ( !( reinterpret_cast<uintptr_t>( p ) & 3 ) ) return *in_hbm<uint32_t>( p );
  const AA_GLOBAL uint8_t * b = in_hbm<uint8_t>( p );
  return uint32_t( b[0] ) | uint32_t( b[1] ) << 8 | uint32_t( b[2] ) << 16 | uint32_t( b[3] ) << 24;
}
// 16 pixels of one row (blocks 0 .. nblk-1 of a tile)
__device__ __forceinline__ void row16( const uint8_t * p, int nblk, bool fast, uint32_t w[4] )
{
  if ( fast ) {
    const u32x4 q = *in_hbm<u32x4>( p );
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    return;
  }
#pragma unroll
  for ( int k = 0; k < 4; k++ ) w[k] = k < nblk ? quad( p + 4 * k ) : 0u;
}

__global__ __launch_bounds__( 256 ) void k_quality_blocks( const aa_quality_job * jobs, float * group_values, unsigned long long * sse )
{
  // block sums: [block row][s1 | s2 << 16, ss, s12][block column].  s1, s2 <= 16 * 255 and a window adds four of them: no carry
  __shared__ uint32_t S[kStripRows + 1][3][kCols];
  __shared__ unsigned long long wave_sse[4];
  const aa_quality_job & J = jobs[blockIdx.y];
  if ( blockIdx.x >= J.strips * J.chunks ) return;
  const int strip = static_cast<int>( blockIdx.x / J.chunks ), chunk = static_cast<int>( blockIdx.x % J.chunks );
  const int w4 = static_cast<int>( J.w4 ), h4 = static_cast<int>( J.h4 );
  const int r0 = strip * kStripRows, c0 = chunk * kChunkWin;
  const int rows = min( kStripRows + 1, h4 - r0 ), cols = min( kCols, w4 - c0 );       // blocks loaded
  const bool last_strip = strip == static_cast<int>( J.strips ) - 1, last_chunk = chunk == static_cast<int>( J.chunks ) - 1;
  const int own_rows = last_strip ? rows : kStripRows, own_cols = last_chunk ? cols : kChunkWin;   // ... and counted for the SSE
  const int tiles = ( cols + 3 ) >> 2;
  const bool aligned = !( ( reinterpret_cast<uintptr_t>( J.a ) | reinterpret_cast<uintptr_t>( J.b ) | static_cast<uintptr_t>( J.stride_a ) | static_cast<uintptr_t>( J.stride_b ) ) & 15 );

  unsigned long long sq = 0;
  for ( int t = threadIdx.x; t < rows * tiles; t += 256 ) {
    const int br = t / tiles, tc = t - br * tiles;
    const int nblk = min( 4, cols - 4 * tc );
    const bool fast = aligned && nblk == 4;
    const int64_t x = 4 * int64_t( c0 + 4 * tc ), y = 4 * int64_t( r0 + br );
    const uint8_t * pa = J.a + y * J.stride_a + x, * pb = J.b + y * J.stride_b + x;
    uint32_t a[4][4], b[4][4];
#pragma unroll
    for ( int i = 0; i < 4; i++ ) { row16( pa + i * J.stride_a, nblk, fast, a[i] ); row16( pb + i * J.stride_b, nblk, fast, b[i] ); }
#pragma unroll
    for ( int k = 0; k < 4; k++ ) {
      uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
#pragma unroll
      for ( int i = 0; i < 4; i++ ) {
        s1 = __builtin_amdgcn_udot4( a[i][k], 0x01010101u, s1, false );
        s2 = __builtin_amdgcn_udot4( b[i][k], 0x01010101u, s2, false );
        ss = __builtin_amdgcn_udot4( a[i][k], a[i][k], ss, false );
        ss = __builtin_amdgcn_udot4( b[i][k], b[i][k], ss, false );
        s12 = __builtin_amdgcn_udot4( a[i][k], b[i][k], s12, false );
      }
      if ( k < nblk ) {
        const int c = 4 * tc + k;
        S[br][0][c] = s1 | s2 << 16; S[br][1][c] = ss; S[br][2][c] = s12;
        if ( br < own_rows && c < own_cols ) sq += ss - 2u * s12;            // sum of (p - q)^2 over the block: never negative
      }
    }
  }
  __syncthreads();

  // windows of this strip and chunk, one thread per group of four
  const int wrows = rows - 1, wins = last_chunk ? cols - 1 : kChunkWin, ngroups = ( wins + 3 ) >> 2;
  for ( int t = threadIdx.x; t < wrows * ngroups; t += 256 ) {
    const int wr = t / ngroups, g = t - wr * ngroups;
    float part = 0.0f;
#pragma unroll
    for ( int k = 0; k < 4; k++ ) {
      const int c = 4 * g + k;
      if ( c >= wins ) break;
      const uint32_t s = S[wr][0][c] + S[wr][0][c + 1] + S[wr + 1][0][c] + S[wr + 1][0][c + 1];
      const int i1 = static_cast<int>( s & 0xFFFFu ), i2 = static_cast<int>( s >> 16 );
      const int iss = static_cast<int>( S[wr][1][c] + S[wr][1][c + 1] + S[wr + 1][1][c] + S[wr + 1][1][c + 1] );
      const int i12 = static_cast<int>( S[wr][2][c] + S[wr][2][c + 1] + S[wr + 1][2][c] + S[wr + 1][2][c + 1] );
      const int c1 = 416, c2 = 235963;             // (int)(.01*.01*255*255*64 + .5), (int)(.03*.03*255*255*64*63 + .5)
      const int vars = iss * 64 - i1 * i1 - i2 * i2, covar = i12 * 64 - i1 * i2;
      const float num = __fmul_rn( static_cast<float>( 2 * i1 * i2 + c1 ), static_cast<float>( 2 * covar + c2 ) );
      const float den = __fmul_rn( static_cast<float>( i1 * i1 + i2 * i2 + c1 ), static_cast<float>( vars + c2 ) );
      part = __fadd_rn( part, __fdiv_rn( num, den ) );
    }
    group_values[J.out_off + uint64_t( r0 + wr ) * J.groups + uint32_t( c0 / 4 + g )] = part;
  }

  if ( !sse ) return;
#pragma unroll
  for ( int d = 32; d > 0; d >>= 1 ) sq += __shfl_xor( sq, d );
  if ( !( threadIdx.x & 63 ) ) wave_sse[threadIdx.x >> 6] = sq;
  __syncthreads();
  if ( threadIdx.x == 0 ) atomicAdd( &sse[blockIdx.y], wave_sse[0] + wave_sse[1] + wave_sse[2] + wave_sse[3] );
}

// x264's summation of a plane's group values (they lie in its order: row after row, group after group) and the mean
__global__ __launch_bounds__( 64 ) void k_quality_sum( const aa_quality_job * jobs, const float * group_values, double * ssim )
{
  __shared__ f32x4 stage[256];
  const aa_quality_job & J = jobs[blockIdx.x];
  const uint32_t count = ( J.h4 - 1 ) * J.groups, nvec = ( count + 3 ) >> 2;
  const AA_GLOBAL f32x4 * src = in_hbm<f32x4>( group_values + J.out_off );            // (out_off is a multiple of 4)
  const uint32_t lane = threadIdx.x;
  // 1024 values at a time: four float4 per lane, the next lot in flight under the chain
  const auto fetch = [&]( uint32_t i ) { f32x4 v = { 0.0f, 0.0f, 0.0f, 0.0f }; if ( i < nvec ) v = src[i]; return v; };
  f32x4 r0 = fetch( lane ), r1 = fetch( lane + 64u ), r2 = fetch( lane + 128u ), r3 = fetch( lane + 192u );
  float total = 0.0f;
  for ( uint32_t base = 0; base < nvec; base += 256 ) {
    stage[lane] = r0; stage[lane + 64u] = r1; stage[lane + 128u] = r2; stage[lane + 192u] = r3;
    __syncthreads();
    const uint32_t next = base + 256u + lane;
    r0 = fetch( next ); r1 = fetch( next + 64u ); r2 = fetch( next + 128u ); r3 = fetch( next + 192u );
    if ( lane == 0 ) {
      const uint32_t m = min( 1024u, count - 4u * base );
      uint32_t i = 0;
      for ( ; i + 4 <= m; i += 4 ) {
        const f32x4 v = stage[i >> 2];
        total = __fadd_rn( total, v.x ); total = __fadd_rn( total, v.y ); total = __fadd_rn( total, v.z ); total = __fadd_rn( total, v.w );
      }
      const float * tail = reinterpret_cast<const float *>( stage );
      for ( ; i < m; i++ ) total = __fadd_rn( total, tail[i] );
    }
    __syncthreads();
  }
  if ( lane == 0 ) ssim[blockIdx.x] = __ddiv_rn( static_cast<double>( total ), static_cast<double>( uint64_t( J.w4 - 1 ) * uint64_t( J.h4 - 1 ) ) );
}

} // namespace

int launch_quality( const aa_quality_job * jobs, int n_planes, uint32_t max_blocks, float * group_values, double * ssim, unsigned long long * sse, void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  for ( int base = 0; base < n_planes; base += 32768 ) {
    const int cnt = std::min( 32768, n_planes - base );
    hipLaunchKernelGGL( k_quality_blocks, dim3( max_blocks, cnt ), dim3( 256 ), 0, st, jobs + base, group_values, sse ? sse + base : nullptr );
    if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  }
  hipLaunchKernelGGL( k_quality_sum, dim3( n_planes ), dim3( 64 ), 0, st, jobs, group_values, ssim );
  return static_cast<int>( hipGetLastError() );
}

} // namespace aa
