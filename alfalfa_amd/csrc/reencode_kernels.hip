// The re-encode (aa_reencode_batch; Encoder::reencode_as_interframe, reencode.cc:38-129): a chunk's key frame encoded again as an inter
// frame predicted from the job stream's CURRENT last reference -- per macroblock the reference's mode decision (intra candidates, the
// B_PRED trial, ZEROMV / NEARESTMV / NEARMV, the diamond search for NEWMV: reencode_search.hh), then the chosen mode applied as the rebase
// applies it (reencode_mb.hh over rebase_inl.hh).  Batched: blockIdx.x is the job (one stream's new frame), jobs are independent.
//
//   k_reencode_inter   ONE workgroup per job, kReencSlots slots of 16 lanes (four waves).  A macroblock needs the modes and vectors of its
//                      left, above and above-left neighbours (census, B_PRED contexts) and the unfiltered reconstruction of its left,
//                      above, above-left and above-right neighbours (intra candidates), so the workgroup walks the 2:1 wavefront
//                      d = col + 2 * row: the macroblocks of one anti-diagonal are independent, a slot takes one of them, and a
//                      workgroup barrier stands between two rounds.  No workgroup talks to another, nothing is polled, no atomics
//                      across workgroups: the row hand-off of k_recon_intra4 is not reused, for k_rebase_intra's reason -- a job is
//                      one frame, and hundreds of jobs fill the machine without it.
//
// Neighbour pixels and side records that ANOTHER wave of the workgroup stored in an earlier round are read from memory with the
// agent-scope loads of k_rebase_intra (load_recon_u32: past the CU's L1), behind __threadfence() + the round's barrier; they are not
// kept in LDS.  A slot's own LDS picture (ReencLds) is private to its 16 lanes, so inside a round nothing but wave-level ordering is
// needed and no slot ever waits for another: slots of one wave run searches of different lengths, and the slot without a macroblock
// in a round is predicated off -- every wave reaches every barrier.
#include "reencode_wave.hh"

namespace aa {

// grid.x = job; slots: how many macroblocks of an anti-diagonal a round takes (1..kReencSlots)
__global__ __launch_bounds__( kReencSlots * 16 ) void k_reencode_inter( const aa_reencode_dev_job * jobs, const int slots )
{
#define AA_WALK_POLICY ReencodePolicy
#include "reencode_walk.inc"
#undef AA_WALK_POLICY
}

int launch_reencode( const aa_reencode_dev_job * jobs, int n, int slots, void * stream )
{
  const hipStream_t st = static_cast<hipStream_t>( stream );
  slots = std::max( 1, std::min( slots, kReencSlots ) );
  hipLaunchKernelGGL( k_reencode_inter, dim3( n ), dim3( kReencSlots * 16 ), 0, st, jobs, slots );
  if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  return 0;
}

} // namespace aa
