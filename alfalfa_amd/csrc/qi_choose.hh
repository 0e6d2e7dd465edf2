// The rule of the target-size quantiser search, host and device (one source): Encoder::encode_with_target_size (encoder.cc:597-628) -- a
// bisection over y_ac_qi in [q_lo, q_hi]: the midpoint's frame size is estimated; a size that fits the target (or the last candidate of a
// search that has found none yet) becomes the choice and the search goes on BELOW it, a size that does not fit sends it ABOVE -- continued
// one candidate at a time, so that a search whose estimates come back in rounds (aa_target_size_batch: one launch per round over every
// unfinished job) visits exactly the candidates the plain loop visits, in its order, and ends where it ends.  The order matters beyond the
// choice: every estimate hands its header carry to the next one.
#pragma once
#include <stdint.h>

#if defined( __HIPCC__ )
#define AA_QIC_HD __host__ __device__ inline __attribute__( ( always_inline ) )
#else
#define AA_QIC_HD inline
#endif

namespace aa {

constexpr int kQiNone = 255;            // best_y_qi before any candidate was taken: numeric_limits<uint8_t>::max()
constexpr int kQiMaxSteps = 8;          // all 128 indices halve to nothing in eight steps; the reference's ranges (at most 4..127) in seven

// A search between rounds.  steps: estimates made so far.
struct QiChoice {
  int32_t lo, hi;                       // y_qi_min, y_qi_max
  int32_t best;                         // best_y_qi (kQiNone: none yet)
  int32_t steps;
};

AA_QIC_HD void qi_choice_begin( QiChoice & c, const int q_lo, const int q_hi ) { c.lo = q_lo; c.hi = q_hi; c.best = kQiNone; c.steps = 0; }
AA_QIC_HD bool qi_choice_done( const QiChoice & c ) { return c.lo > c.hi; }
// the candidate the next estimate is made for (only while the search is not done)
AA_QIC_HD int qi_choice_candidate( const QiChoice & c ) { return ( c.lo + c.hi ) / 2; }

// One step: `estimated_size` is the estimate for qi_choice_candidate( c ).
AA_QIC_HD void qi_choice_step( QiChoice & c, const uint64_t estimated_size, const uint64_t target_size )
{
  const int q = qi_choice_candidate( c );
  c.steps++;
  if ( estimated_size <= target_size || ( c.lo == c.hi && c.best == kQiNone ) ) { c.best = q; c.hi = q - 1; }
  else c.lo = q + 1;
}

// The range the search starts from (encoder.cc:597-608): [4, 127], or around the last frame's index where the encoder keeps one (real-time
// quality only): last - 16 where that is not below 4, and last + 16 capped at 127.  last_q < 0: none.
AA_QIC_HD void qi_target_range( const int last_q, int & q_lo, int & q_hi )
{
  q_lo = 4; q_hi = 127;
  if ( last_q < 0 ) return;
  if ( last_q - 16 >= q_lo ) q_lo = last_q - 16;
  q_hi = q_hi < last_q + 16 ? q_hi : last_q + 16;
}

} // namespace aa
