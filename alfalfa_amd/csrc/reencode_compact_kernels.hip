// The re-encode's records compacted where they lie (aa_reencode_device_batch): behind k_reencode_inter, on the same stream, the records,
// masks and dense slots the decision left in the slice's piece become each frame's records and dense blocks in parse order, in the
// frame's own piece of HBM -- what reencode_records (runtime_reencode.inc) builds on the host after a download.  The pair of
// rebase_compact_kernels.hip (same grid: blockIdx.y the job, blockIdx.x a run of kCompactMbs macroblocks, a thread per macroblock; same
// statements, compact_device.hh) with what the re-encode adds, by the rule of reencode_compact.hh: the input records are the decision's
// own, so the host knows no mode --
//
//   k_reencode_count     beside the run's stored-block population (one word per (job, run) into `partials`) the frame's intra-row words:
//                        a frame has fewer words than macroblocks, so word w is the thread's whose macroblock is w -- it reads the
//                        ref_frame of the word's (at most 64) records and stores the word, into the slice's piece.  Every word has one
//                        writer; rows may straddle runs, no workgroup needs another's.  The host fetches sums and words with one copy
//                        and derives the intra count, the diagonals and the piece's size.
//   k_reencode_compact   k_rebase_compact with lf_level set per macroblock (mb_lf_level over the job's HeaderParams in the second
//                        table); the row words it copies into the frame's piece are the device copy the count pass made.
// No atomics.  Every loop is bounded by the job's macroblock count.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "compact_device.hh"
#include "reencode_compact.hh"

namespace aa {

namespace {

using compact::kCompactThreads;
using compact::kCompactWaves;

struct ReencodeRecord {
  const HeaderParams * fp;
  __device__ __forceinline__ aa_mb_info operator()( const aa_mb_info & m, const uint32_t raw, const uint32_t index ) const { return compact::reencode_record( m, raw, index, *fp ); }
};

} // namespace

__global__ __launch_bounds__( kCompactThreads ) void k_reencode_count( const aa_reencode_dev_job * jobs, uint32_t * partials, uint32_t stride )
{
  __shared__ uint32_t wave_sum[kCompactWaves];
  const aa_reencode_dev_job & J = jobs[blockIdx.y];
  const uint32_t mbw = J.base.mbw, total = mbw * J.base.mbh;
  const uint32_t first = blockIdx.x * compact::kCompactMbs;
  if ( first >= total ) return;                             // (whole workgroup: jobs of one call may differ in size)
  const uint32_t mi = first + threadIdx.x;
  if ( mi < compact::row_words( mbw, J.base.mbh ) ) J.intra_rows[mi] = compact::intra_row_word( J.mbs_out, mbw, mi );
  const uint32_t n = mi < total ? compact::popc( compact::stored_mask( J.base.masks[mi], J.mbs_out[mi].y_mode ) ) : 0u;
  compact::run_sum( n, wave_sum, partials + static_cast<size_t>( blockIdx.y ) * stride + blockIdx.x );
}

__global__ __launch_bounds__( kCompactThreads ) void k_reencode_compact( const aa_reencode_dev_job * jobs, const aa_rebase_compact_job * outs, const HeaderParams * lf,
                                                                         const uint32_t * partials, uint32_t stride )
{
  __shared__ uint32_t run_mask[kCompactThreads], run_index[kCompactThreads];
  __shared__ uint32_t wave_sum[kCompactWaves];
  const aa_reencode_dev_job & J = jobs[blockIdx.y];
  const uint32_t total = static_cast<uint32_t>( J.base.mbw ) * J.base.mbh;
  if ( blockIdx.x * compact::kCompactMbs >= total ) return;
  compact::compact_run( J.mbs_out, J.base.masks, J.base.coeffs, total, outs[blockIdx.y], partials + static_cast<size_t>( blockIdx.y ) * stride, run_mask, run_index, wave_sum,
                        ReencodeRecord { lf + blockIdx.y } );
}

int launch_reencode_count( const aa_reencode_dev_job * jobs, int n, uint32_t max_mbs, uint32_t * partials, uint32_t stride, void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  for ( int base = 0; base < n; base += 32768 ) {
    const int cnt = std::min( 32768, n - base );
    hipLaunchKernelGGL( k_reencode_count, dim3( compact::runs_of( max_mbs ), cnt ), dim3( kCompactThreads ), 0, st, jobs + base, partials + static_cast<size_t>( base ) * stride, stride );
    if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  }
  return 0;
}

int launch_reencode_compact( const aa_reencode_dev_job * jobs, const aa_rebase_compact_job * outs, const void * lf, int n, uint32_t max_mbs, const uint32_t * partials, uint32_t stride,
                             void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  const HeaderParams * params = static_cast<const HeaderParams *>( lf );
  for ( int base = 0; base < n; base += 32768 ) {
    const int cnt = std::min( 32768, n - base );
    hipLaunchKernelGGL( k_reencode_compact, dim3( compact::runs_of( max_mbs ), cnt ), dim3( kCompactThreads ), 0, st, jobs + base, outs + base, params + base,
                        partials + static_cast<size_t>( base ) * stride, stride );
    if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  }
  return 0;
}

} // namespace aa
