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

#include "compact_device.hh"      // the statements shared with the re-encode's pair (reencode_compact_kernels.hip)

namespace aa {

namespace {

using compact::kCompactThreads;
using compact::kCompactWaves;

// a rebased frame's output record: the input's with the residue fields set
struct RebaseRecord {
  __device__ __forceinline__ aa_mb_info operator()( const aa_mb_info & m, const uint32_t raw, const uint32_t index ) const { return compact::output_record( m, raw, index ); }
};

} // namespace

__global__ __launch_bounds__( kCompactThreads ) void k_rebase_count( const aa_rebase_dev_job * jobs, uint32_t * partials, uint32_t stride )
{
  __shared__ uint32_t wave_sum[kCompactWaves];
  const aa_rebase_dev_job & J = jobs[blockIdx.y];
  const uint32_t total = static_cast<uint32_t>( J.mbw ) * J.mbh;
  const uint32_t first = blockIdx.x * compact::kCompactMbs;
  if ( first >= total ) return;                             // (whole workgroup: jobs of one call may differ in size)
  const uint32_t mi = first + threadIdx.x;
  const uint32_t n = mi < total ? compact::popc( compact::stored_mask( J.masks[mi], J.mbs[mi].y_mode ) ) : 0u;
  compact::run_sum( n, wave_sum, partials + static_cast<size_t>( blockIdx.y ) * stride + blockIdx.x );
}

__global__ __launch_bounds__( kCompactThreads ) void k_rebase_compact( const aa_rebase_dev_job * jobs, const aa_rebase_compact_job * outs, const uint32_t * partials, uint32_t stride )
{
  __shared__ uint32_t run_mask[kCompactThreads], run_index[kCompactThreads];
  __shared__ uint32_t wave_sum[kCompactWaves];
  const aa_rebase_dev_job & J = jobs[blockIdx.y];
  const uint32_t total = static_cast<uint32_t>( J.mbw ) * J.mbh;
  if ( blockIdx.x * compact::kCompactMbs >= total ) return;
  compact::compact_run( J.mbs, J.masks, J.coeffs, total, outs[blockIdx.y], partials + static_cast<size_t>( blockIdx.y ) * stride, run_mask, run_index, wave_sum, RebaseRecord() );
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
