// The loop-filter level search of appended frames, batched (aa_lf_search_decode_batch, runtime_lf_batch.inc): every job's frame has been
// reconstructed once, unfiltered, into its own raster; a ROUND tries up to AA_LF_MAX_ROUND consecutive levels per job that is still
// searching.  Between the launches of this file run what exists: one k_loopfilter_rows4 over all candidates of the round and one
// k_quality_blocks / k_quality_sum over their luma planes.
//
//   k_lf_candidates   blockIdx.y = an entry of the round's table (a job and its n candidate levels), blockIdx.x strides over the job's
//                     raster in 16-byte pieces: a piece is loaded ONCE and stored to each of the n candidate rasters (consecutive
//                     threads take consecutive pieces: whole lines both ways).  Then the same threads stride over the job's 80-byte
//                     records, five pieces each, k_lf_relevel's statement per candidate: the first piece carries lf_level, which becomes
//                     the candidate's level of the record's segment.  The first workgroup's first n threads write the candidates' job
//                     records: the job's own with the candidate's planes, records and level.  A candidate of level 0 gets nothing: it is
//                     the unfiltered raster itself.
//   k_lf_choose       a thread per entry continues the rule of lf_choose.hh over the round's scores (measure 1: made from the integer
//                     squared error first); the state of every search stays in device memory.
//   k_lf_finish       blockIdx.y = a job: the chosen level into the job's own records (by segment) and job record, in place.
// Plain grids: no LDS, no atomics, no polling; every loop is bounded by the plane size, the macroblock count or AA_LF_MAX_ROUND.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "device_types.h"

namespace aa {

namespace {
constexpr int kLfThreads = 256;

// an 80-byte record's first piece (y_mode uv_mode ref_frame segment_id | flags lf_level ...) with lf_level from `levels`
__device__ __forceinline__ uint4 relevel( uint4 head, const uint32_t levels )
{
  head.y = lf_relevel_word( head.x, head.y, levels );
  return head;
}
} // namespace

static_assert( sizeof( aa_mb_info ) == 80, "five 16-byte pieces per record" );
static_assert( sizeof( aa_dev_frame ) % 8 == 0, "job records are copied as a struct" );

__global__ __launch_bounds__( kLfThreads ) void k_lf_candidates( const aa_lf_search_dev_job * jobs, const aa_lf_round_entry * entries )
{
  const aa_lf_round_entry E = entries[blockIdx.y];
  const aa_lf_search_dev_job & J = jobs[E.job];
  const uint32_t n = min( E.n, static_cast<uint32_t>( AA_LF_MAX_ROUND ) );
  const aa_dev_frame * const F = J.frame;
  const uint32_t stride = gridDim.x * kLfThreads, t0 = blockIdx.x * kLfThreads + threadIdx.x;

  // ---- the raster: one load, a store per candidate ----
  const uint4 * const src = reinterpret_cast<const uint4 *>( F->cur[0] );
  const uint32_t n16 = J.raster_bytes >> 4;
  for ( uint32_t i = t0; i < n16; i += stride ) {
    const uint4 v = src[i];
    for ( uint32_t c = 0; c < n; c++ )
      if ( E.first_level + static_cast<int>( c ) != 0 ) reinterpret_cast<uint4 *>( J.cand + c * J.per )[i] = v;
  }
  // ---- the records ----
  const uint4 * const rec = reinterpret_cast<const uint4 *>( F->mbs );
  const uint32_t pieces = J.nmb * 5u;
  for ( uint32_t i = t0; i < pieces; i += stride ) {
    const uint4 v = rec[i];
    const bool head = i % 5u == 0;
    for ( uint32_t c = 0; c < n; c++ ) {
      const int level = E.first_level + static_cast<int>( c );
      if ( level == 0 ) continue;
      reinterpret_cast<uint4 *>( J.cand + c * J.per + J.records_off )[i] = head ? relevel( v, lf_segment_levels( J.seg, level ) ) : v;
    }
  }
  // ---- the job records ----
  if ( blockIdx.x == 0 && threadIdx.x < n ) {
    const int level = E.first_level + static_cast<int>( threadIdx.x );
    if ( level != 0 ) {
      uint8_t * const base = J.cand + threadIdx.x * J.per;
      // (word by word and then the fields that differ, through the pointer: a local copy of the struct would be private memory)
      aa_dev_frame * const f = reinterpret_cast<aa_dev_frame *>( base + J.job_off );
      const uint64_t * const from = reinterpret_cast<const uint64_t *>( F );
      uint64_t * const to = reinterpret_cast<uint64_t *>( f );
      for ( uint32_t w = 0; w < sizeof( aa_dev_frame ) / 8; w++ ) to[w] = from[w];
      f->cur[0] = base; f->cur[1] = base + J.luma_bytes; f->cur[2] = base + J.luma_bytes + J.chroma_bytes;
      f->mbs = reinterpret_cast<const aa_mb_info *>( base + J.records_off );
      f->loop_filter_level = static_cast<uint8_t>( level );
    }
  }
}

__global__ __launch_bounds__( 64 ) void k_lf_choose( const aa_lf_search_dev_job * jobs, const aa_lf_round_entry * entries, int n_entries, const double * ssim,
                                                     const unsigned long long * sse, int measure, LfChoice * states )
{
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if ( e >= n_entries ) return;
  const aa_lf_round_entry E = entries[e];
  const aa_lf_search_dev_job & J = jobs[E.job];
  LfChoice c = states[E.job];
  const int n = static_cast<int>( min( E.n, static_cast<uint32_t>( AA_LF_MAX_ROUND ) ) );
  for ( int i = 0; i < n; i++ ) {
    const double q = measure ? lf_sse_score( sse[E.score_off + i], J.pw, J.ph ) : ssim[E.score_off + i];
    lf_choice_round( c, E.first_level + i, &q, 1, J.level_hi );
  }
  states[E.job] = c;
}

__global__ __launch_bounds__( kLfThreads ) void k_lf_finish( const aa_lf_search_dev_job * jobs, const LfChoice * states )
{
  const aa_lf_search_dev_job & J = jobs[blockIdx.y];
  aa_dev_frame * const F = J.frame;
  const int level = states[blockIdx.y].best_level;
  const uint32_t levels = lf_segment_levels( J.seg, level );
  uint4 * const rec = reinterpret_cast<uint4 *>( const_cast<aa_mb_info *>( F->mbs ) );
  for ( uint32_t i = blockIdx.x * kLfThreads + threadIdx.x; i < J.nmb; i += gridDim.x * kLfThreads ) rec[i * 5u] = relevel( rec[i * 5u], levels );
  if ( blockIdx.x == 0 && threadIdx.x == 0 ) F->loop_filter_level = static_cast<uint8_t>( level );
}

int launch_lf_candidates( const aa_lf_search_dev_job * jobs, const aa_lf_round_entry * entries, int n_entries, uint32_t max_raster_bytes, void * stream )
{
  // 16 pieces per thread where the raster is large; a job's workgroups all take part in its records too
  const unsigned per = static_cast<unsigned>( std::min<size_t>( 64, std::max<size_t>( 1, max_raster_bytes / ( kLfThreads * 16 * 16 ) ) ) );
  const hipStream_t st = static_cast<hipStream_t>( stream );
  for ( int base = 0; base < n_entries; base += 32768 ) {
    hipLaunchKernelGGL( k_lf_candidates, dim3( per, std::min( 32768, n_entries - base ) ), dim3( kLfThreads ), 0, st, jobs, entries + base );
    if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  }
  return 0;
}

int launch_lf_choose( const aa_lf_search_dev_job * jobs, const aa_lf_round_entry * entries, int n_entries, const double * ssim, const unsigned long long * sse, int measure,
                      LfChoice * states, void * stream )
{
  hipLaunchKernelGGL( k_lf_choose, dim3( ( n_entries + 63 ) / 64 ), dim3( 64 ), 0, static_cast<hipStream_t>( stream ), jobs, entries, n_entries, ssim, sse, measure, states );
  return static_cast<int>( hipGetLastError() );
}

int launch_lf_finish( const aa_lf_search_dev_job * jobs, const LfChoice * states, int n_jobs, uint32_t max_mbs, void * stream )
{
  const unsigned per = std::max( 1u, std::min( 64u, ( max_mbs + kLfThreads - 1 ) / kLfThreads ) );
  const hipStream_t st = static_cast<hipStream_t>( stream );
  for ( int base = 0; base < n_jobs; base += 32768 ) {
    hipLaunchKernelGGL( k_lf_finish, dim3( per, std::min( 32768, n_jobs - base ) ), dim3( kLfThreads ), 0, st, jobs + base, states + base );
    if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  }
  return 0;
}

} // namespace aa
