// The second pass of a key frame (aa_encode_two_pass_batch / aa_encode_two_pass_device_batch; encode_raster<KeyFrame> with two_pass_encoder_,
// encode_intra.cc:409-439), behind k_encode_key (encode_kernels.hip), which is the first pass and is not touched:
//
//   k_encode_key2    Key2Policy: a key frame's SECOND pass (aa_encode_two_pass_batch; encode_intra.cc:409-439) over what k_encode_key left --
//                    the decision again, every quantisation the trellis's (trellis_quant.hh: sixteen lanes build the sixteen luma
//                    trellises of a 16x16 mode at once, the picks are settled in block order; the B_PRED trial stays serial), check_reset_y2 in
//                    front of the Y2 block.  Between the passes, over the first pass's raw output (key2_first_pass.hh):
//   k_key2_first_pass   per macroblock the two side bits the second pass reads, and the first pass's token branch counts (k_token_counts'
//                       scheme: LDS atomics, one round of vector atomics per workgroup)
//   k_key2_updates      one thread per probability: the first pass's token_prob_update, which the reference keeps wherever the
//                       second pass makes no update of its own
//
// The schedule is k_encode_key's (reencode_walk.inc): one workgroup per job, kReencSlots slots of 16 lanes, the 2:1 wavefront.  A file of
// its own: encode_kernels.hip holds the single-pass encoder's two kernels and nothing else.
#include "reencode_wave.hh"
#include "key2_first_pass.hh"

namespace aa {

__global__ __launch_bounds__( kReencSlots * 16 ) void k_encode_key2( const aa_reencode_dev_job * jobs, const int slots )
{
#define AA_WALK_POLICY Key2Policy
#define AA_WALK_LANES DevLanes2
#include "reencode_walk.inc"
#undef AA_WALK_LANES
#undef AA_WALK_POLICY
}

constexpr uint32_t kKey2Run = 64;       // macroblocks per workgroup of k_key2_first_pass

// workgroup (x, job): macroblocks [x * kKey2Run, (x + 1) * kKey2Run) of the job's frame, sixteen at a time, 16 lanes each: lane b counts luma
// block b, lanes 0..7 then the chroma blocks 16 + b; lane 0 writes the macroblock's side bits
__global__ __launch_bounds__( 256 ) void k_key2_first_pass( const aa_reencode_dev_job * jobs )
{
  __shared__ uint32_t cnt[2112];
  const aa_reencode_dev_job & J = jobs[blockIdx.y];
  const EncKey2Costs & C = *static_cast<const EncKey2Costs *>( J.costs );
  const uint32_t mbw = J.base.mbw, nmb = static_cast<uint32_t>( J.base.mbw ) * J.base.mbh;
  const uint32_t begin = blockIdx.x * kKey2Run, end = begin + kKey2Run < nmb ? begin + kKey2Run : nmb;
  if ( begin >= nmb ) return;                                        // (the whole workgroup)
  for ( uint32_t i = threadIdx.x; i < 2112; i += 256 ) cnt[i] = 0;
  __syncthreads();
  const uint32_t b16 = threadIdx.x & 15u, slot = threadIdx.x >> 4;
  for ( uint32_t m0 = begin; m0 < end; m0 += 16 ) {
    const uint32_t mi = m0 + slot;
    if ( mi >= end ) continue;
    if ( b16 == 0 ) const_cast<uint8_t *>( C.first_pass )[mi] = first_pass_bits( J.mbs_out[mi], J.base.masks[mi] );
    for ( uint32_t b = b16; b < 24; b += 16 )
      count_raw_block( [&]( const uint32_t node, const uint32_t taken ) { atomicAdd( &cnt[2u * node + taken], 1u ); }, J.mbs_out, J.base.masks, J.base.coeffs, mbw, mi, b );
  }
  __syncthreads();
  for ( uint32_t i = threadIdx.x; i < 2112; i += 256 ) if ( cnt[i] ) atomicAdd( &C.counts[i], cnt[i] );
}

__global__ __launch_bounds__( 256 ) void k_key2_updates( const aa_reencode_dev_job * jobs )
{
  const EncKey2Costs & C = *static_cast<const EncKey2Costs *>( jobs[blockIdx.y].costs );
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if ( i >= 1056 ) return;
  uint8_t flag, value;
  key_update( C.counts[2 * i], C.counts[2 * i + 1], k_default_coeff_probs[i], flag, value );
  C.updates[i] = flag; C.updates[1056 + i] = value;
}

// the steps between a two-pass key job's first pass (k_encode_key, launched with the other key jobs) and its end
int launch_encode_second_pass( const aa_reencode_dev_job * jobs, int n, uint32_t max_mbs, int slots, void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  if ( n <= 0 || !max_mbs ) return static_cast<int>( hipErrorInvalidValue );
  slots = std::max( 1, std::min( slots, kReencSlots ) );
  hipLaunchKernelGGL( k_key2_first_pass, dim3( ( max_mbs + kKey2Run - 1 ) / kKey2Run, n ), dim3( 256 ), 0, st, jobs );
  if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  hipLaunchKernelGGL( k_key2_updates, dim3( 5, n ), dim3( 256 ), 0, st, jobs );
  if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  hipLaunchKernelGGL( k_encode_key2, dim3( n ), dim3( kReencSlots * 16 ), 0, st, jobs, slots );
  if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  return 0;
}

} // namespace aa
