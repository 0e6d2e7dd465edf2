// The rebase's records compacted where they lie (aa_rebase_device_batch): behind k_rebase_inter / k_rebase_intra, on the same stream, the
// masks and dense slots of a slice become each frame's records and dense blocks in parse order, in the frame's own piece of HBM --
// what rebase_records (runtime_rebase.inc) builds on the host after a download, by the rule of rebase_compact.hh.  Batched like the
// rebase kernels: blockIdx.y is the job, blockIdx.x a run of kCompactMbs macroblocks, one thread per macroblock; jobs of one launch may
// differ in size, a workgroup past its job's end returns.
//
//   k_rebase_count     the population of every stored mask, summed per run: a wave reduction by shuffles, four words of LDS, one word per
//                      (job, run) into `partials`.  The host sums a job's words into num_coeff_blocks and allocates the frame's piece.
//   k_rebase_compact   a run's first coeff_index is the sum of the words of the runs before it (a few dozen uniform loads; no workgroup
//                      waits for another, nothing polls); an exclusive scan of the run's 256 populations -- wave scans by shuffles, the
//                      wave totals in LDS -- gives every macroblock's; each thread writes its record (five 16-byte stores); then the
//                      workgroup copies the run's 256 x 25 slots as 16-byte halves, thread t taking halves t, t + 256, ...: a half whose
//                      slot's mask bit is clear is skipped before its load, the others go to (coeff_index + place in parse order) * 32
//                      + half * 16 of the frame's coefficient area.  The run's masks and indices sit in LDS.  Run 0 also writes the
//                      frame's job record and intra-row words from what the host put into the job table.
// No atomics.  Every loop is bounded by the job's macroblock count.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "device_types.h"
#include "rebase_compact.hh"

namespace aa {

namespace {

constexpr int kCompactThreads = static_cast<int>( compact::kCompactMbs );
constexpr int kCompactWaves = kCompactThreads / 64;
static_assert( sizeof( aa_mb_info ) == 80 && sizeof( aa_dev_frame ) % 16 == 0 && sizeof( aa_dev_frame ) / 16 <= kCompactThreads, "records and job record move as 16-byte units" );

union RecordUnits { aa_mb_info mb; uint4 q[5]; };

} // namespace

__global__ __launch_bounds__( kCompactThreads ) void k_rebase_count( const aa_rebase_dev_job * jobs, uint32_t * partials, uint32_t stride )
{
  __shared__ uint32_t wave_sum[kCompactWaves];
  const aa_rebase_dev_job & J = jobs[blockIdx.y];
  const uint32_t total = static_cast<uint32_t>( J.mbw ) * J.mbh;
  const uint32_t first = blockIdx.x * compact::kCompactMbs;
  if ( first >= total ) return;                             // (whole workgroup: jobs of one call may differ in size)
  const uint32_t mi = first + threadIdx.x;
  uint32_t n = mi < total ? compact::popc( compact::stored_mask( J.masks[mi], J.mbs[mi].y_mode ) ) : 0u;
#pragma unroll
  for ( int off = 32; off; off >>= 1 ) n += __shfl_down( n, off );
  if ( ( threadIdx.x & 63 ) == 0 ) wave_sum[threadIdx.x >> 6] = n;
  __syncthreads();
  if ( threadIdx.x == 0 ) {
    uint32_t sum = 0;
#pragma unroll
    for ( int w = 0; w < kCompactWaves; w++ ) sum += wave_sum[w];
    partials[static_cast<size_t>( blockIdx.y ) * stride + blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__( kCompactThreads ) void k_rebase_compact( const aa_rebase_dev_job * jobs, const aa_rebase_compact_job * outs, const uint32_t * partials, uint32_t stride )
{
  __shared__ uint32_t run_mask[kCompactThreads], run_index[kCompactThreads];
  __shared__ uint32_t wave_sum[kCompactWaves];
  const aa_rebase_dev_job & J = jobs[blockIdx.y];
  const aa_rebase_compact_job & O = outs[blockIdx.y];
  const uint32_t total = static_cast<uint32_t>( J.mbw ) * J.mbh;
  const uint32_t first = blockIdx.x * compact::kCompactMbs;
  if ( first >= total ) return;
  const uint32_t in_run = total - first < compact::kCompactMbs ? total - first : compact::kCompactMbs;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t base = compact::run_base( partials + static_cast<size_t>( blockIdx.y ) * stride, blockIdx.x );

  // ---- this thread's macroblock: record in, stored mask, its place in the frame by a scan of the run ----
  const uint32_t mi = first + tid;
  const bool have = mi < total;
  RecordUnits R;
  uint32_t raw = 0;
  if ( have ) {
    const uint4 * src = reinterpret_cast<const uint4 *>( J.mbs + mi );
#pragma unroll
    for ( int k = 0; k < 5; k++ ) R.q[k] = src[k];
    raw = J.masks[mi];
  } else {
#pragma unroll
    for ( int k = 0; k < 5; k++ ) R.q[k] = make_uint4( 0, 0, 0, 0 );
  }
  const uint32_t mask = compact::stored_mask( raw, R.mb.y_mode );
  const uint32_t n = compact::popc( mask );
  uint32_t incl = n;
#pragma unroll
  for ( int off = 1; off < 64; off <<= 1 ) {
    const uint32_t v = __shfl_up( incl, off );
    if ( lane >= static_cast<uint32_t>( off ) ) incl += v;
  }
  if ( lane == 63 ) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t before = base;
#pragma unroll
  for ( int w = 0; w < kCompactWaves; w++ ) if ( static_cast<uint32_t>( w ) < wave ) before += wave_sum[w];
  const uint32_t index = before + incl - n;
  run_mask[tid] = mask; run_index[tid] = index;
  if ( have ) {
    R.mb = compact::output_record( R.mb, raw, index );
    uint4 * dst = reinterpret_cast<uint4 *>( O.out_mbs + mi );
#pragma unroll
    for ( int k = 0; k < 5; k++ ) dst[k] = R.q[k];
  }
  // ---- run 0: the frame's job record and intra-row words ----
  if ( blockIdx.x == 0 ) {
    if ( tid < sizeof( aa_dev_frame ) / 16 ) reinterpret_cast<uint4 *>( O.out_frame )[tid] = reinterpret_cast<const uint4 *>( &O.frame )[tid];
    for ( uint32_t w = tid; w < O.rows_words; w += kCompactThreads ) O.out_rows[w] = O.rows[w];
  }
  __syncthreads();

  // ---- the run's slots, 16 bytes a thread and trip ----
  const uint8_t * dense = reinterpret_cast<const uint8_t *>( J.coeffs ) + static_cast<size_t>( first ) * AA_REBASE_MB_BYTES;
  uint8_t * blocks = reinterpret_cast<uint8_t *>( O.out_coeffs );
  const uint32_t units = in_run * compact::kUnitsPerMb;
  for ( uint32_t u = tid; u < units; u += kCompactThreads ) {
    const compact::Unit x = compact::unit_of( u );
    const uint32_t m = run_mask[x.mb];
    if ( !compact::unit_stored( x, m ) ) continue;
    const uint32_t block = compact::unit_block( x, m, run_index[x.mb] );
    if ( block >= O.num_coeff_blocks ) continue;            // (cannot happen while the host's sum is this kernel's: nothing is ever stored outside the piece)
    const uint4 v = *reinterpret_cast<const uint4 *>( dense + compact::unit_source( x ) );
    *reinterpret_cast<uint4 *>( blocks + static_cast<size_t>( block ) * 32 + x.half * 16 ) = v;
  }
}

int launch_rebase_count( const aa_rebase_dev_job * jobs, int n, uint32_t max_mbs, uint32_t * partials, uint32_t stride, void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  for ( int base = 0; base < n; base += 32768 ) {
    const int cnt = std::min( 32768, n - base );
    hipLaunchKernelGGL( k_rebase_count, dim3( compact::runs_of( max_mbs ), cnt ), dim3( kCompactThreads ), 0, st, jobs + base, partials + static_cast<size_t>( base ) * stride, stride );
    if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  }
  return 0;
}

int launch_rebase_compact( const aa_rebase_dev_job * jobs, const aa_rebase_compact_job * outs, int n, uint32_t max_mbs, const uint32_t * partials, uint32_t stride, void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  for ( int base = 0; base < n; base += 32768 ) {
    const int cnt = std::min( 32768, n - base );
    hipLaunchKernelGGL( k_rebase_compact, dim3( compact::runs_of( max_mbs ), cnt ), dim3( kCompactThreads ), 0, st, jobs + base, outs + base, partials + static_cast<size_t>( base ) * stride, stride );
    if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  }
  return 0;
}

} // namespace aa
