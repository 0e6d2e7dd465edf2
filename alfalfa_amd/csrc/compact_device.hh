// The device statements the two pairs of compaction kernels share -- k_rebase_count / k_rebase_compact (rebase_compact_kernels.hip) and
// k_reencode_count / k_reencode_compact (reencode_compact_kernels.hip): the sum of a run's populations, and a run compacted into the
// frame's piece by the rule of rebase_compact.hh.  A kernel names where its job's records, masks and dense slots lie and how an output
// record is made of an input record; the LDS is the kernel's own and handed in.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "rebase_compact.hh"

namespace aa {
namespace compact {

constexpr int kCompactThreads = static_cast<int>( kCompactMbs );
constexpr int kCompactWaves = kCompactThreads / 64;
static_assert( sizeof( aa_mb_info ) == 80 && sizeof( aa_dev_frame ) % 16 == 0 && sizeof( aa_dev_frame ) / 16 <= kCompactThreads, "records and job record move as 16-byte units" );

union RecordUnits { aa_mb_info mb; uint4 q[5]; };

// The workgroup's sum of `n` (a thread's stored blocks) -> *out, by thread 0: a wave reduction by shuffles, the wave sums (kCompactWaves
// words of LDS) added up.
__device__ __forceinline__ void run_sum( uint32_t n, uint32_t * wave_sum, uint32_t * out )
{
#pragma unroll
  for ( int off = 32; off; off >>= 1 ) n += __shfl_down( n, off );
  if ( ( threadIdx.x & 63 ) == 0 ) wave_sum[threadIdx.x >> 6] = n;
  __syncthreads();
  if ( threadIdx.x == 0 ) {
    uint32_t sum = 0;
#pragma unroll
    for ( int w = 0; w < kCompactWaves; w++ ) sum += wave_sum[w];
    *out = sum;
  }
}

// Run blockIdx.x of a job of `total` macroblocks (the caller has checked that the run exists): records `mbs`, raw masks `masks`, dense
// slots `coeffs` -> O's piece.  partials: the job's words of the count pass.  record( input record, raw mask, coeff_index ) -> the
// output record.  run_mask, run_index: kCompactThreads words of LDS each; wave_sum: kCompactWaves.
template <class Record>
__device__ __forceinline__ void compact_run( const aa_mb_info * mbs, const uint32_t * masks, const int16_t * coeffs, const uint32_t total, const aa_rebase_compact_job & O,
                                             const uint32_t * partials, uint32_t * run_mask, uint32_t * run_index, uint32_t * wave_sum, const Record & record )
{
  const uint32_t first = blockIdx.x * kCompactMbs;
  const uint32_t in_run = total - first < kCompactMbs ? total - first : kCompactMbs;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t base = run_base( partials, blockIdx.x );

  // ---- this thread's macroblock: record in, stored mask, its place in the frame by a scan of the run ----
  const uint32_t mi = first + tid;
  const bool have = mi < total;
  RecordUnits R;
  uint32_t raw = 0;
  if ( have ) {
    const uint4 * src = reinterpret_cast<const uint4 *>( mbs + mi );
#pragma unroll
    for ( int k = 0; k < 5; k++ ) R.q[k] = src[k];
    raw = masks[mi];
  } else {
#pragma unroll
    for ( int k = 0; k < 5; k++ ) R.q[k] = make_uint4( 0, 0, 0, 0 );
  }
  const uint32_t mask = stored_mask( raw, R.mb.y_mode );
  const uint32_t n = popc( mask );
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
    R.mb = record( R.mb, raw, index );
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
  const uint8_t * dense = reinterpret_cast<const uint8_t *>( coeffs ) + static_cast<size_t>( first ) * AA_REBASE_MB_BYTES;
  uint8_t * blocks = reinterpret_cast<uint8_t *>( O.out_coeffs );
  const uint32_t units = in_run * kUnitsPerMb;
  for ( uint32_t u = tid; u < units; u += kCompactThreads ) {
    const Unit x = unit_of( u );
    const uint32_t m = run_mask[x.mb];
    if ( !unit_stored( x, m ) ) continue;
    const uint32_t block = unit_block( x, m, run_index[x.mb] );
    if ( block >= O.num_coeff_blocks ) continue;            // (cannot happen while the host's sum is the count pass's: nothing is ever stored outside the piece)
    const uint4 v = *reinterpret_cast<const uint4 *>( dense + unit_source( x ) );
    *reinterpret_cast<uint4 *>( blocks + static_cast<size_t>( block ) * 32 + x.half * 16 ) = v;
  }
}

} // namespace compact
} // namespace aa
