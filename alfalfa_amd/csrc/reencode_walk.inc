// The body of k_reencode_inter, k_encode_key and k_encode_inter: one workgroup, one job (jobs[blockIdx.x]) -- the anti-diagonals
// d = col + 2 * row in turn, `slots` macroblocks of one per round (1..kReencSlots), a workgroup barrier between two rounds.  Included
// inside the kernel, with AA_WALK_POLICY = the policy of the decision (reencode_search.hh): the text is the kernel's own, so the three
// kernels differ by nothing but the policy, and k_reencode_inter compiles to what it was before it had siblings.
// AA_WALK_LANES (optional): the lanes' type where it is not DevLanes.
#if !defined( AA_WALK_LANES )
#define AA_WALK_LANES DevLanes
#define AA_WALK_LANES_DEFAULTED
#endif
  __shared__ ReencLds lds[kReencSlots];
  const aa_reencode_dev_job & J = jobs[blockIdx.x];
  const int slot = threadIdx.x >> 4;
  const int mbw = J.base.mbw, mbh = J.base.mbh;
  AA_WALK_LANES lanes;
  lanes.b = threadIdx.x & 15;
  const int last = ( mbw - 1 ) + 2 * ( mbh - 1 );
  for ( int d = 0; d <= last; d++ ) {
    // rows of the anti-diagonal: col = d - 2 * row in [0, mbw)
    const int row_lo = d > mbw - 1 ? ( d - ( mbw - 1 ) + 1 ) / 2 : 0, row_hi = std::min( mbh - 1, d / 2 );
    const int count = row_hi - row_lo + 1;
    for ( int base = 0; base < count; base += slots ) {
      const int k = base + slot;
      if ( slot < slots && k < count ) {
        const int row = row_lo + k, col = d - 2 * row;
        ReencMb<AA_WALK_LANES, AA_WALK_POLICY> mb( lanes, J, lds[slot], static_cast<size_t>( row ) * mbw + col );
        mb.run();
      }
      __threadfence();            // the next rounds' macroblocks read this round's pixels and side records back from memory
      __syncthreads();
    }
  }
#if defined( AA_WALK_LANES_DEFAULTED )
#undef AA_WALK_LANES
#undef AA_WALK_LANES_DEFAULTED
#endif
