// Hashes of rasters and segment maps, batched and device-resident (aa_hash_rasters_async / aa_hash_decoders_async): the reference's
// boost::hash_range chain (hash_chain.hh) cannot be split, but chains are independent of each other -- one lane walks one chain, as
// the token lanes do for the entropy decode.
//
//   k_hash_chains   lane l < lanes_per_wave of workgroup g (one wave) walks job g * lanes_per_wave + l: 16 bytes per load with the
//                   next two in flight, 16 dependent steps of 7 VALU instructions each per load.  The kernel is bound by one wave's
//                   instruction issue, so a lane alone in its wave is as fast as 64: the host gives every SIMD of the chip a wave
//                   before any wave gets a second lane, and sorts the jobs by length so that the lanes of a wave finish together.
//                   No LDS, no atomics, nothing between lanes; each result is one 8-byte vector store into the call's result table
//                   (pinned host memory).
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "hash_chain.hh"

namespace aa {
namespace {

__global__ __launch_bounds__( 64 ) void k_hash_chains( const HashJob * jobs, uint32_t n, uint32_t lanes_per_wave, uint64_t * results )
{
  if ( threadIdx.x >= lanes_per_wave ) return;
  const uint32_t i = blockIdx.x * lanes_per_wave + threadIdx.x;
  if ( i >= n ) return;
  const HashJob j = jobs[i];
  if ( j.out_index < n ) results[j.out_index] = hash_job_walk( j );       // (the table has n words)
}

} // namespace

int launch_hash_chains( const HashJob * jobs, int n, int lanes_per_wave, uint64_t * results, void * stream )
{
  if ( n <= 0 || lanes_per_wave < 1 || lanes_per_wave > 64 ) return static_cast<int>( hipErrorInvalidValue );
  const unsigned waves = ( static_cast<unsigned>( n ) + lanes_per_wave - 1 ) / lanes_per_wave;
  hipLaunchKernelGGL( k_hash_chains, dim3( waves ), dim3( 64 ), 0, static_cast<hipStream_t>( stream ), jobs, static_cast<uint32_t>( n ),
                      static_cast<uint32_t>( lanes_per_wave ), results );
  return static_cast<int>( hipGetLastError() );
}

} // namespace aa
