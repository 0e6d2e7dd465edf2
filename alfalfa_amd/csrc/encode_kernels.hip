// The forward encoder (aa_encode_batch; Encoder::encode_with_quantizer, encoder.cc:559-575): a raster encoded as a key frame
// (encode_raster<KeyFrame>, encode_intra.cc:388-456) or as an inter frame predicted from the job stream's current last reference
// (encode_raster<InterFrame>, encode_inter.cc:577-653), first pass.  The macroblock code is the re-encode's (reencode_mb.hh) under the two
// forward policies of the decision (reencode_search.hh); the schedule is k_reencode_inter's (reencode_walk.inc): one workgroup per job,
// kReencSlots slots of 16 lanes, the 2:1 wavefront, __threadfence() and a workgroup barrier between rounds, neighbours' pixels and side
// records re-read past L1, nothing polled, no atomics across workgroups.
//
//   k_encode_key     KeyPolicy: the intra candidates with the key frame's mode costs, the B_PRED trial in both qualities.  No inter
//                    candidate is instantiated: no reference plane is read, no census taken, and its cost block (EncKeyCosts, 2 KB) holds
//                    neither the probability costs nor the 8 KB of vector costs.
//   k_encode_inter   ForwardInterPolicy: the re-encode's candidates with the job's multipliers, and a diamond search whose sites cost their
//                    SAD plus the rate of their vector (EncInterCosts).
//
// A call that mixes kinds launches each kernel once over its own job table.
#include "reencode_wave.hh"

namespace aa {

__global__ __launch_bounds__( kReencSlots * 16 ) void k_encode_key( const aa_reencode_dev_job * jobs, const int slots )
{
#define AA_WALK_POLICY KeyPolicy
#include "reencode_walk.inc"
#undef AA_WALK_POLICY
}

__global__ __launch_bounds__( kReencSlots * 16 ) void k_encode_inter( const aa_reencode_dev_job * jobs, const int slots )
{
#define AA_WALK_POLICY ForwardInterPolicy
#include "reencode_walk.inc"
#undef AA_WALK_POLICY
}

int launch_encode( const aa_reencode_dev_job * jobs, int n, bool key, int slots, void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  slots = std::max( 1, std::min( slots, kReencSlots ) );
  if ( key ) hipLaunchKernelGGL( k_encode_key, dim3( n ), dim3( kReencSlots * 16 ), 0, st, jobs, slots );
  else hipLaunchKernelGGL( k_encode_inter, dim3( n ), dim3( kReencSlots * 16 ), 0, st, jobs, slots );
  if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  return 0;
}

} // namespace aa
