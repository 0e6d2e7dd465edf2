// The frame-size estimate (aa_estimate_size_batch, and every round of aa_target_size_batch; Encoder::estimate_frame_size,
// size_estimation.cc): the forward encoder's first pass over every fourth macroblock of a picture in each direction, as a small frame of
// its own, and the size that frame serialises to.
//
//   k_estimate_key     EstimateKeyPolicy / EstimateInterPolicy (reencode_search.hh): k_encode_key's and k_encode_inter's decisions and
//   k_estimate_inter   macroblock code under kSampled (reencode_mb.hh) -- macroblock (c, r) of the job's small frame reads the original at
//                      (4c, 4r), searches and predicts its candidates at that position of the full-size reference, and reconstructs at
//                      (c, r), where an inter macroblock predicts AGAIN from the small frame's position.  The schedule is k_reencode_inter's
//                      (reencode_walk.inc): one workgroup per job, the 2:1 wavefront over the small frame, a barrier between rounds.
//   k_estimate_tokens  a lane per job behind them: the small frame's one DCT partition walked with a boolean encoder that counts and
//                      stores nothing (estimate_size.hh over serialize_common.hh), straight from the decision's records, masks and dense
//                      coefficient slots.  -> the partition's bytes and what the host's header needs: macroblocks with coefficients, intra
//                      macroblocks.  As with k_serialize_tokens a lane is a chain of dependent integer instructions: `lanes_per_wave` spreads
//                      the jobs over the chip's SIMDs.
//
// Nothing but those three words per job, the masks and the records the first partition is written from comes down: never frame bytes.
#include "reencode_wave.hh"
#include "estimate_size.hh"

namespace aa {

__global__ __launch_bounds__( kReencSlots * 16 ) void k_estimate_key( const aa_reencode_dev_job * jobs, const int slots )
{
#define AA_WALK_POLICY EstimateKeyPolicy
#include "reencode_walk.inc"
#undef AA_WALK_POLICY
}

__global__ __launch_bounds__( kReencSlots * 16 ) void k_estimate_inter( const aa_reencode_dev_job * jobs, const int slots )
{
#define AA_WALK_POLICY EstimateInterPolicy
#include "reencode_walk.inc"
#undef AA_WALK_POLICY
}

__global__ __launch_bounds__( 64 ) void k_estimate_tokens( const aa_reencode_dev_job * jobs, const aa_estimate_dev_job * sizes, const uint32_t n, const uint32_t lanes_per_wave )
{
  if ( threadIdx.x >= lanes_per_wave ) return;
  const uint32_t i = blockIdx.x * lanes_per_wave + threadIdx.x;
  if ( i >= n ) return;
  const aa_reencode_dev_job & J = jobs[i];
  BoolWriter w;                                   // no capacity: every byte is counted, none stored
  const est::Counts c = est::write_tokens( w, sizes[i].token_probs, J.mbs_out, J.base.masks, J.base.coeffs, J.base.mbw, J.base.mbh );
  uint32_t * out = sizes[i].result;
  out[0] = c.token_bytes; out[1] = c.with_coefficients; out[2] = c.intra; out[3] = 0;
}

int launch_estimate( const aa_reencode_dev_job * jobs, int n, bool key, int slots, void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  slots = std::max( 1, std::min( slots, kReencSlots ) );
  if ( key ) hipLaunchKernelGGL( k_estimate_key, dim3( n ), dim3( kReencSlots * 16 ), 0, st, jobs, slots );
  else hipLaunchKernelGGL( k_estimate_inter, dim3( n ), dim3( kReencSlots * 16 ), 0, st, jobs, slots );
  if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  return 0;
}

int launch_estimate_tokens( const aa_reencode_dev_job * jobs, const aa_estimate_dev_job * sizes, int n, int lanes_per_wave, void * stream )
{
  if ( n <= 0 || lanes_per_wave < 1 || lanes_per_wave > 64 ) return static_cast<int>( hipErrorInvalidValue );
  const unsigned waves = ( static_cast<unsigned>( n ) + lanes_per_wave - 1 ) / lanes_per_wave;
  hipLaunchKernelGGL( k_estimate_tokens, dim3( waves ), dim3( 64 ), 0, static_cast<hipStream_t>( stream ), jobs, sizes, static_cast<uint32_t>( n ),
                      static_cast<uint32_t>( lanes_per_wave ) );
  return static_cast<int>( hipGetLastError() );
}

} // namespace aa
