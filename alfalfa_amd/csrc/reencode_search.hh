// The decision of the re-encode (aa_reencode_batch; Encoder::reencode_as_interframe, reencode.cc:38-129): which prediction a macroblock
// of the new inter frame gets.  The rate model (costs.cc), the candidate order and the tie-breaks of luma_mb_best_prediction_mode /
// luma_mb_inter_predict (encode_intra.cc:83-161, encode_inter.cc:231-369), diamond_search and its outer loop (encode_inter.cc:172-229,
// 287-298), all in the reference's integer types.  No pixel is touched here: SAD, variance and the B_PRED trial sit behind the `Px`
// argument, so the kernel answers them with sixteen lanes and the host simulation (tests/cpp/reencode_sim.cc) with loops.  Marked AA_MHD
// like vp8_math.hh: host and device compile one source.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstring>

#include "cost_tables.h"
#include "parse_common.hh"
#include "trellis_quant.hh"
#include "vp8_math.hh"
#include "vp8_tables.h"

namespace aa {

enum : int { REENC_BEST = 0, REENC_REALTIME = 1 };
constexpr uint32_t kRateMultiplier = 300, kDistortionMultiplier = 1;     // encoder.hh:152-153 (update_rd_multipliers is the second pass's)
constexpr uint32_t kNoCost = 0xFFFFFFFFu;                                // MBPredictionData's initial cost, encoder.hh:103-105

// Everything of the rate model a job's macroblocks read, built on the host (reenc_fill_costs), one per job in device memory.
struct ReencCosts {
  uint16_t prob_cost[256];          // cost of a bool of probability p / 256 (costs.cc:18; cost_tables.h)
  uint16_t bmode[10][10][10];       // [above][left][mode], from kf_b_mode_probs (Costs::fill_mode_costs)
  uint16_t mbmode_intra[5];         // mbmode_costs[1][DC_PRED .. B_PRED], from k_default_y_mode_probs
  uint16_t mv_comp[2][2][1024];     // [row, column][negative][magnitude], from the stream's CURRENT motion-vector probabilities
  uint8_t mv_counts_to_probs[24];
  uint8_t quality, pad[5];
};
static_assert( sizeof( ReencCosts ) % 8 == 0, "ReencCosts sits in a table of 8-byte aligned pieces" );

// Encoder::rdcost (encoder.cc:410-416): uint32_t arithmetic as written
AA_MHD uint32_t rdcost( uint32_t rate, uint32_t distortion, uint32_t rate_multiplier, uint32_t distortion_multiplier )
{
  return ( ( 128u + rate * rate_multiplier ) / 256u ) + distortion * distortion_multiplier;
}

AA_MHD uint16_t cost_bit( const uint16_t * prob_cost, uint8_t prob, int bit ) { return prob_cost[bit ? 255 - prob : prob]; }

// Costs::compute_cost (costs.cc:151-170): the cost of every leaf of a tree, costs[-leaf]; uint16_t sums as there.  The trees here are
// at most nine nodes deep, so the recursion is an explicit stack.
AA_MHD void tree_costs( uint16_t * costs, const uint8_t * probs, const int8_t * tree, const uint16_t * prob_cost )
{
  int node[10]; uint16_t cost[10];
  int top = 0;
  node[0] = 0; cost[0] = 0;
  while ( top >= 0 ) {
    const int at = node[top]; const uint16_t sofar = cost[top];
    top--;
    for ( int i = 0; i < 2; i++ ) {
      const int entry = tree[at + i];
      const uint16_t c = static_cast<uint16_t>( sofar + cost_bit( prob_cost, probs[at / 2], i ) );
      if ( entry <= 0 ) costs[-entry] = c;
      else { top++; node[top] = entry; cost[top] = c; }
    }
  }
}

// The inter entries of mbmode_costs[1] (Costs::fill_mv_ref_costs): mv_ref_tree is a chain, so its leaves' costs are running sums
// (SPLITMV is never a candidate here).  Four named values, not an array: a run-time index would put it into private memory on the GPU.
struct MvRefCosts { uint16_t zero, nearest, near, newmv; };
AA_MHD MvRefCosts mv_ref_costs( const uint8_t ( &probs )[4], const uint16_t * prob_cost )
{
  MvRefCosts c;
  uint16_t ones = 0;
  c.zero = cost_bit( prob_cost, probs[0], 0 ); ones = cost_bit( prob_cost, probs[0], 1 );
  c.nearest = static_cast<uint16_t>( ones + cost_bit( prob_cost, probs[1], 0 ) ); ones = static_cast<uint16_t>( ones + cost_bit( prob_cost, probs[1], 1 ) );
  c.near = static_cast<uint16_t>( ones + cost_bit( prob_cost, probs[2], 0 ) ); ones = static_cast<uint16_t>( ones + cost_bit( prob_cost, probs[2], 1 ) );
  c.newmv = static_cast<uint16_t>( ones + cost_bit( prob_cost, probs[3], 0 ) );
  return c;
}

// Costs::mv_component_cost (costs.cc:76-111)
AA_MHD uint32_t mv_component_cost( int16_t num, const uint8_t * probs, const uint16_t * prob_cost )
{
  enum { IS_SHORT, SIGN, SHORT, BITS = SHORT + 8 - 1, LONG_MV_WIDTH = 10 };
  const int16_t num_to_encode = static_cast<int16_t>( num >> 1 );
  const uint16_t x = static_cast<uint16_t>( num_to_encode < 0 ? -num_to_encode : num_to_encode );
  uint32_t cost;
  if ( x < 8 ) {
    uint16_t tree = 0;                 // tree_cost( x, 3, small_mv_tree, probs.slice<SHORT, 7>() ), costs.cc:58-73
    int index = 0;
    for ( int n = 3; n-- > 0; ) {
      const int bit = ( x >> n ) & 1;
      tree = static_cast<uint16_t>( tree + cost_bit( prob_cost, probs[SHORT + index / 2], bit ) );
      index = kSmallMvTree[index + bit];
    }
    cost = prob_cost[probs[IS_SHORT]] + tree;
  } else {
    cost = prob_cost[255 - probs[IS_SHORT]];
    for ( int i = 0; i < 3; i++ ) cost += cost_bit( prob_cost, probs[BITS + i], ( x >> i ) & 1 );
    for ( int i = LONG_MV_WIDTH - 1; i > 3; i-- ) cost += cost_bit( prob_cost, probs[BITS + i], ( x >> i ) & 1 );
    if ( x & 0xfff0 ) cost += cost_bit( prob_cost, probs[BITS + 3], ( x >> 3 ) & 1 );
  }
  return cost;
}

// Costs::motion_vector_cost (costs.cc:222-226); the vector is a difference from best_ref and stays within +-1023 on this path
AA_MHD uint32_t motion_vector_cost( const ReencCosts & C, int x, int y, uint32_t weight )
{
  const int ax = iabs( x ) & 1023, ay = iabs( y ) & 1023;
  return static_cast<uint32_t>( ( static_cast<uint64_t>( C.mv_comp[0][y < 0][ay] ) + C.mv_comp[1][x < 0][ax] ) * weight / 128u );
}

// ---- the three policies of the decision: whose rate model, which multipliers, what a site of the diamond search costs ----
// EncInterCosts / EncKeyCosts: the cost blocks of the forward encoder (aa_encode_batch; Encoder::encode_raster, encode_inter.cc:577-653,
// encode_intra.cc:388-456), filled on the host (enc_fill_inter_costs / enc_fill_key_costs).  The multipliers are update_rd_multipliers'
// (encoder.cc:178-193), per job.
struct EncInterCosts {
  ReencCosts base;                  // mode, sub-block mode and vector costs as the re-encode's
  uint32_t rate_mul, dist_mul;
  uint32_t sad_per_bit;             // sad_per_bit16lut[y_ac_qi], the weight of a site's rate
  uint32_t pad;
  uint16_t mv_sad[256];             // Costs::fill_mv_sad_costs (costs.cc:135-149)
};
static_assert( sizeof( EncInterCosts ) % 8 == 0, "EncInterCosts sits in a table of 8-byte aligned pieces" );
// A key frame reads no probability, no vector cost and no census table: two kilobytes, not ten
struct EncKeyCosts {
  uint16_t bmode[10][10][10];       // as ReencCosts'
  uint16_t mbmode[5];               // mbmode_costs[0][DC_PRED .. B_PRED], from k_kf_y_mode_probs over kKfYModeTree
  uint16_t pad;
  uint32_t rate_mul, dist_mul;
  uint32_t pad2;
};
static_assert( sizeof( EncKeyCosts ) % 8 == 0, "EncKeyCosts sits in a table of 8-byte aligned pieces" );

// Costs::sad_motion_vector_cost( mv, MotionVector(), weight ) (costs.cc:231-240)
AA_MHD uint32_t sad_motion_vector_cost( const uint16_t * mv_sad, int mvx, int mvy, uint32_t weight )
{
  int x = mvx >> 2, y = mvy >> 2;
  x = x > 255 ? 255 : ( x < -255 ? -255 : x ); y = y > 255 ? 255 : ( y < -255 ? -255 : y );
  return static_cast<uint32_t>( ( ( static_cast<uint64_t>( mv_sad[iabs( y )] ) + mv_sad[iabs( x )] ) * weight + 128u ) / 256u );
}

// aa_reencode_batch: Encoder::reencode_as_interframe.  Constants 300 / 1; a site of the search costs its SAD (see diamond_search).
struct ReencodePolicy {
  using Costs = ReencCosts;
  static constexpr bool kKey = false, kSampled = false;
  static constexpr bool kSecondPass = false;
  AA_MHD static uint32_t rate_mul( const Costs & ) { return kRateMultiplier; }
  AA_MHD static uint32_t dist_mul( const Costs & ) { return kDistortionMultiplier; }
  AA_MHD static const uint16_t * bmode( const Costs & C, int above, int left ) { return C.bmode[above][left]; }
  AA_MHD static uint32_t mbmode_intra( const Costs & C, int mode ) { return C.mbmode_intra[mode]; }
  AA_MHD static bool tries_bpred( const Costs & C ) { return C.quality != REENC_REALTIME; }
  AA_MHD static const ReencCosts & inter( const Costs & C ) { return C; }
  AA_MHD static uint32_t site_cost( const Costs &, int, int, uint32_t sad ) { return rdcost( 0, sad, 1, 1 ); }
};
// aa_encode_batch, an inter frame: encode_raster<InterFrame>.  The job's multipliers; a site costs its SAD and the rate of its vector.
struct ForwardInterPolicy {
  using Costs = EncInterCosts;
  static constexpr bool kKey = false, kSampled = false;
  static constexpr bool kSecondPass = false;
  AA_MHD static uint32_t rate_mul( const Costs & C ) { return C.rate_mul; }
  AA_MHD static uint32_t dist_mul( const Costs & C ) { return C.dist_mul; }
  AA_MHD static const uint16_t * bmode( const Costs & C, int above, int left ) { return C.base.bmode[above][left]; }
  AA_MHD static uint32_t mbmode_intra( const Costs & C, int mode ) { return C.base.mbmode_intra[mode]; }
  AA_MHD static bool tries_bpred( const Costs & C ) { return C.base.quality != REENC_REALTIME; }
  AA_MHD static const ReencCosts & inter( const Costs & C ) { return C.base; }
  AA_MHD static uint32_t site_cost( const Costs & C, int mvx, int mvy, uint32_t sad ) { return rdcost( sad_motion_vector_cost( C.mv_sad, mvx, mvy, C.sad_per_bit ), sad, 1, 1 ); }
};
// aa_encode_batch, a key frame: encode_raster<KeyFrame>.  No inter candidate; the B_PRED trial in both qualities (the real-time
// exclusion, encode_intra.cc:98-102, is the inter frames' alone).
struct KeyPolicy {
  using Costs = EncKeyCosts;
  static constexpr bool kKey = true, kSampled = false;
  static constexpr bool kSecondPass = false;
  AA_MHD static uint32_t rate_mul( const Costs & C ) { return C.rate_mul; }
  AA_MHD static uint32_t dist_mul( const Costs & C ) { return C.dist_mul; }
  AA_MHD static const uint16_t * bmode( const Costs & C, int above, int left ) { return C.bmode[above][left]; }
  AA_MHD static uint32_t mbmode_intra( const Costs & C, int mode ) { return C.mbmode[mode]; }
  AA_MHD static bool tries_bpred( const Costs & ) { return true; }
};

// aa_encode_two_pass_batch, a key frame's SECOND pass (encode_raster<KeyFrame> with two_pass_encoder_, encode_intra.cc:409-439): the key
// frame's decision over again, every quantisation the trellis's (trellis_quant.hh) and check_reset_y2 in front of the Y2 block's.  The job's
// cost block carries, behind the first pass's, the token costs and what the first pass left behind per macroblock (k_key2_first_pass):
//   bit 0   the first pass chose B_PRED: the type its Y blocks ended with, which the second pass's B_PRED trial meets (the trial quantises
//           BEFORE it sets the type, encode_intra.cc:62-66) -- after a 16x16 mode the trial's trellis starts at position 1, under the
//           Y-after-Y2 costs, and leaves the block's unquantised DC where it is
//   bit 1   the first pass's Y2 block held a coefficient: the flag a macroblock that is B_PRED in the second pass keeps (an uncoded Y2
//           block is not recomputed, encoder.cc:636), and which the Y2 trellis of the macroblocks to its right and below reads as context
struct EncKey2Costs {
  EncKeyCosts enc;
  const TrellisCosts * trellis;
  const uint8_t * first_pass;       // [mbw * mbh]
  uint32_t * counts;                // [2112]: the first pass's branch counts [4][8][3][11][2] {false, true}; zeroed by the host
  uint8_t * updates;                // [2112]: the first pass's 1056 update flags, then its 1056 values (k_key2_updates)
  uint32_t * census;                // host simulation only (tests/cpp/encode2_sim.cc): counts of the cases met; null in a job of the kernel's
};
static_assert( sizeof( EncKey2Costs ) % 8 == 0, "EncKey2Costs sits in a table of 8-byte aligned pieces" );
// (the cases the host simulation counts: a walk that kept another level than the truncated quotient or an earlier end; a Y2 block
// check_reset_y2 emptied; B_PRED chosen after a 16x16 mode of the first pass; a Y2 trellis that ran beside a B_PRED macroblock, whose flag
// is the first pass's; the same with that flag set)
enum : int { K2_TRELLIS_NOT_TRUNCATED, K2_Y2_RESET, K2_BPRED_AFTER_16X16, K2_STALE_Y2_CONTEXT, K2_STALE_Y2_SET, K2_CENSUS };
struct Key2Policy {
  using Costs = EncKey2Costs;
  static constexpr bool kKey = true, kSampled = false;
  static constexpr bool kSecondPass = true;
  AA_MHD static uint32_t rate_mul( const Costs & C ) { return C.enc.rate_mul; }
  AA_MHD static uint32_t dist_mul( const Costs & C ) { return C.enc.dist_mul; }
  AA_MHD static const uint16_t * bmode( const Costs & C, int above, int left ) { return C.enc.bmode[above][left]; }
  AA_MHD static uint32_t mbmode_intra( const Costs & C, int mode ) { return C.enc.mbmode[mode]; }
  AA_MHD static bool tries_bpred( const Costs & ) { return true; }
  AA_MHD static void note( const Costs & C, int what )
  {
#if !defined( __HIP_DEVICE_COMPILE__ )
    if ( C.census ) C.census[what]++;
#else
    (void)C; (void)what;
#endif
  }
};

// aa_estimate_size_batch / aa_target_size_batch: Encoder::estimate_size (size_estimation.cc) -- the forward encoder's first pass over
// every fourth macroblock in each direction, as a frame of its own.  The decisions are the forward policies'; kSampled tells the macroblock
// code (reencode_mb.hh) that the job's frame is the SMALL one: macroblock (c, r) of it encodes the original's macroblock (4c, 4r), searches
// and predicts its candidates at that position of the full-size reference, and reconstructs at (c, r).  The cost block carries the
// original's size in macroblocks behind the forward encoder's block.
struct EstInterCosts { EncInterCosts enc; uint32_t full_mbw, full_mbh; };
struct EstKeyCosts { EncKeyCosts enc; uint32_t full_mbw, full_mbh; };
static_assert( sizeof( EstInterCosts ) % 8 == 0 && sizeof( EstKeyCosts ) % 8 == 0, "the estimate's cost blocks sit in a table of 8-byte aligned pieces" );
struct EstimateInterPolicy {
  using Costs = EstInterCosts;
  static constexpr bool kKey = false, kSampled = true;
  static constexpr bool kSecondPass = false;
  AA_MHD static uint32_t rate_mul( const Costs & C ) { return C.enc.rate_mul; }
  AA_MHD static uint32_t dist_mul( const Costs & C ) { return C.enc.dist_mul; }
  AA_MHD static const uint16_t * bmode( const Costs & C, int above, int left ) { return C.enc.base.bmode[above][left]; }
  AA_MHD static uint32_t mbmode_intra( const Costs & C, int mode ) { return C.enc.base.mbmode_intra[mode]; }
  AA_MHD static bool tries_bpred( const Costs & C ) { return C.enc.base.quality != REENC_REALTIME; }
  AA_MHD static const ReencCosts & inter( const Costs & C ) { return C.enc.base; }
  AA_MHD static uint32_t site_cost( const Costs & C, int mvx, int mvy, uint32_t sad ) { return ForwardInterPolicy::site_cost( C.enc, mvx, mvy, sad ); }
  AA_MHD static int full_mbw( const Costs & C ) { return static_cast<int>( C.full_mbw ); }
  AA_MHD static int full_mbh( const Costs & C ) { return static_cast<int>( C.full_mbh ); }
  // the four pixels above-right of a macroblock of the small frame's last column, row >= 1, which no estimate writes (reencode_mb.hh): zero
  AA_MHD static uint32_t unwritten_pixels( const Costs &, int ) { return 0; }
};
struct EstimateKeyPolicy {
  using Costs = EstKeyCosts;
  static constexpr bool kKey = true, kSampled = true;
  static constexpr bool kSecondPass = false;
  AA_MHD static uint32_t rate_mul( const Costs & C ) { return C.enc.rate_mul; }
  AA_MHD static uint32_t dist_mul( const Costs & C ) { return C.enc.dist_mul; }
  AA_MHD static const uint16_t * bmode( const Costs & C, int above, int left ) { return C.enc.bmode[above][left]; }
  AA_MHD static uint32_t mbmode_intra( const Costs & C, int mode ) { return C.enc.mbmode[mode]; }
  AA_MHD static bool tries_bpred( const Costs & ) { return true; }
  AA_MHD static int full_mbw( const Costs & C ) { return static_cast<int>( C.full_mbw ); }
  AA_MHD static int full_mbh( const Costs & C ) { return static_cast<int>( C.full_mbh ); }
  // the four pixels above-right of a macroblock of the small frame's last column, row >= 1, which no estimate writes (reencode_mb.hh): zero
  AA_MHD static uint32_t unwritten_pixels( const Costs &, int ) { return 0; }
};

// luma_sb_intra_predict (encode_intra.cc:360-386): the ten modes ascending, strict <
template <class P = ReencodePolicy>
AA_MHD int pick_bmode( const typename P::Costs & C, const uint16_t * mode_costs, const uint32_t ( &sse )[10], uint32_t & best_sse )
{
  uint32_t min_error = kNoCost;
  int best = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
  for ( int m = 0; m < 10; m++ ) {
    const uint32_t e = rdcost( mode_costs[m], sse[m], P::rate_mul( C ), P::dist_mul( C ) );
    if ( e < min_error ) { best = m; min_error = e; best_sse = sse[m]; }
  }
  return best;
}

// chroma_mb_best_prediction_mode (encode_intra.cc:248-284): by DISTORTION alone, ascending, strict <
AA_MHD int pick_uv_mode( const uint32_t ( &sse )[4] )
{
  uint32_t best_d = kNoCost;
  int best = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
  for ( int m = 0; m < 4; m++ ) if ( sse[m] < best_d ) { best = m; best_d = sse[m]; }
  return best;
}

// What a macroblock's census needs of a neighbour, and what the B_PRED trial of the macroblocks to the right and below needs of
// it (the reference keeps the trial's sub-block modes in the frame even where another mode wins: encode_intra.cc:65,134).
struct ReencNeighbour {
  uint32_t mv;          // x | y << 16: the base vector of an inter-coded macroblock
  uint32_t inter;       // 1: inter-coded
  uint32_t bm_bottom;   // sub-block modes 12..15, a byte each
  uint32_t bm_right;    // sub-block modes 3, 7, 11, 15
};

// Scorer (scorer.hh, macroblock.cc:143-174,301-312) over above, left, above-left -- the statements of parse_mb_header's census
// (parse_common.hh) with every neighbour on LAST -- and what luma_mb_inter_predict takes from it (encode_inter.cc:259-267)
struct ReencCensus {
  Mv best, nearest, near;      // clamped
  uint8_t probs[4];
};
// (Scorer's two arrays of four, indexed by a running count, are named values here: an index known only at run time would put them
// into private memory on the GPU)
struct CensusTally { int s0 = 0, s1 = 0, s2 = 0, s3 = 0, idx = 0; Mv c1, c2, c3; };
AA_MHD Mv census_last( const CensusTally & t ) { return t.idx == 1 ? t.c1 : ( t.idx == 2 ? t.c2 : ( t.idx == 3 ? t.c3 : Mv() ) ); }
AA_MHD void census_add( const ReencNeighbour & nb, int weight, CensusTally & t )
{
  if ( !nb.inter ) return;
  Mv mv; mv.x = static_cast<int16_t>( nb.mv & 0xFFFFu ); mv.y = static_cast<int16_t>( nb.mv >> 16 );
  if ( mv.zero() ) { t.s0 += weight; return; }
  // (every value is written every time, chosen by value: a store through a chosen ADDRESS is a run-time index again)
  const int idx = t.idx + ( mv == census_last( t ) ? 0 : 1 );
  const bool fresh = idx != t.idx;
  t.c1 = fresh && idx == 1 ? mv : t.c1; t.c2 = fresh && idx == 2 ? mv : t.c2; t.c3 = fresh && idx == 3 ? mv : t.c3;
  t.s1 += idx == 1 ? weight : 0; t.s2 += idx == 2 ? weight : 0; t.s3 += idx == 3 ? weight : 0;
  t.idx = idx;
}
// (a neighbour beyond the frame's edge is given as one that is not inter-coded)
AA_MHD ReencCensus census( const ReencNeighbour & above, const ReencNeighbour & left, const ReencNeighbour & above_left, const uint8_t * mv_counts_to_probs,
                           unsigned col, unsigned row, unsigned mbw, unsigned mbh )
{
  CensusTally t;
  census_add( above, 2, t );
  census_add( left, 2, t );
  census_add( above_left, 1, t );
  if ( t.s3 && census_last( t ) == t.c1 ) t.s1 += t.s3;
  if ( t.s2 > t.s1 ) {
    const int ts = t.s1; t.s1 = t.s2; t.s2 = ts;
    const Mv tm = t.c1; t.c1 = t.c2; t.c2 = tm;
  }
  Mv best;
  if ( t.s1 >= t.s0 ) best = t.c1;
  ReencCensus c;
  c.best = clamp_mv( best, col, row, mbw, mbh ); c.nearest = clamp_mv( t.c1, col, row, mbw, mbh ); c.near = clamp_mv( t.c2, col, row, mbw, mbh );
  // (no neighbour is SPLITMV: the fourth count is zero)
  c.probs[0] = mv_counts_to_probs[t.s0 * 4 + 0]; c.probs[1] = mv_counts_to_probs[t.s1 * 4 + 1];
  c.probs[2] = mv_counts_to_probs[t.s2 * 4 + 2]; c.probs[3] = mv_counts_to_probs[0 * 4 + 3];
  return c;
}

AA_MHD bool mv_out_of_bounds( int x, int y ) { return x > 1023 || x < -1023 || y > 1023 || y < -1023; }      // encode_inter.cc:36-47

struct ReencSearch { Mv mv; int first_step; };

// Encoder::diamond_search (encode_inter.cc:172-229).  The step halves from at most 512 down to 2: nine rounds at the most, written
// as a counted loop; a round whose step has run out does nothing.  base: best_ref, already clamped (clamping it again changes nothing).
template <class P = ReencodePolicy, class Px>
AA_MHD ReencSearch diamond_search( Px & px, const typename P::Costs & C, const Mv base, Mv origin, int step_size, unsigned col, unsigned row, unsigned mbw, unsigned mbh )
{
  int first_step = step_size / 2;
  for ( int round = 0; round < 9; round++ ) {
    if ( step_size <= 1 ) continue;
    uint32_t best_cost = kNoCost;
    Mv best;                            // (a round in which every site is out of bounds leaves the default vector)
    for ( int site = 0; site < 5; site++ ) {
      // check_sites: { -1, 0 } { 0, -1 } { 0, 0 } { 0, 1 } { 1, 0 }
      const int sx = site == 0 ? -1 : ( site == 4 ? 1 : 0 ), sy = site == 1 ? -1 : ( site == 3 ? 1 : 0 );
      Mv mv;
      mv.x = static_cast<int16_t>( origin.x + static_cast<int16_t>( step_size * sx ) ); mv.y = static_cast<int16_t>( origin.y + static_cast<int16_t>( step_size * sy ) );
      if ( mv_out_of_bounds( mv.x, mv.y ) ) continue;           // tested BEFORE the base is added
      Mv at; at.x = static_cast<int16_t>( mv.x + base.x ); at.y = static_cast<int16_t>( mv.y + base.y );
      at = clamp_mv( at, col, row, mbw, mbh );
      const uint32_t sad = px.inter_sad( at.x, at.y );
      // rdcost( sad_motion_vector_cost( mv, 0, sad_per_bit16lut[y_ac_qi] ), SAD, 1, 1 ).  On the RE-ENCODE's path the rate is ZERO: Costs is
      // value-initialised (encoder.cc:77,86) and fill_mv_sad_costs is encode_raster's alone (encode_inter.cc:602), which a re-encode never
      // runs, so every entry of mv_sad_costs is 0 and ( 0 * weight + 128 ) / 256 = 0: a site costs its SAD.  The forward encoder fills it.
      const uint32_t cost = P::site_cost( C, mv.x, mv.y, sad );
      if ( cost < best_cost ) { best_cost = cost; best = mv; }
    }
    if ( best == origin ) first_step = step_size / 2;
    origin = best;
    step_size /= 2;
  }
  ReencSearch r; r.mv = origin; r.first_step = first_step;
  return r;
}

// The NEWMV search of luma_mb_inter_predict (encode_inter.cc:287-300): diamond_search again from where it ended, with the step it
// returned, until the vector no longer moves.  The returned step at least halves every time: nine searches at the most.
template <class P = ReencodePolicy, class Px>
AA_MHD Mv newmv_search( Px & px, const typename P::Costs & C, const Mv best_ref, unsigned col, unsigned row, unsigned mbw, unsigned mbh )
{
  Mv mv;
  int step = 512;
  bool done = false;
  for ( int search = 0; search < 9; search++ ) {
    if ( done || step <= 1 ) continue;
    const ReencSearch r = diamond_search<P>( px, C, best_ref, mv, step, col, row, mbw, mbh );
    if ( r.mv == mv ) { done = true; continue; }
    mv = r.mv;
    step = r.first_step;
  }
  mv.x = static_cast<int16_t>( mv.x + best_ref.x ); mv.y = static_cast<int16_t>( mv.y + best_ref.y );
  return mv;
}

struct ReencChoice { int mode; Mv mv; };

// luma_mb_best_prediction_mode( interframe = true ) then the inter candidates of luma_mb_inter_predict.  Px answers:
//   bpred_trial( rate, distortion )   the B_PRED trial: every sub-block picks its mode (pick_bmode), is quantised and reconstructed
//                                     before the next one predicts; rate = the sum of the modes' costs, distortion = the sum of
//                                     the sub-blocks' SSE against the PREDICTION
//   intra_variance( mode )            variance of target - 16x16 prediction
//   inter_sad / inter_variance( x, y ) of target - the luma prediction from LAST at that vector
template <class P = ReencodePolicy, class Px>
AA_MHD ReencChoice choose_prediction( Px & px, const typename P::Costs & C, const ReencCensus & cen, unsigned col, unsigned row, unsigned mbw, unsigned mbh )
{
  uint32_t best_cost = kNoCost;
  ReencChoice best; best.mode = DC_PRED;
  const uint32_t rate_mul = P::rate_mul( C ), dist_mul = P::dist_mul( C );
  // ---- intra: B_PRED first (an inter frame: best quality only), then TM, H, V, DC ----
  if ( P::tries_bpred( C ) ) {
    uint32_t rate = 0, distortion = 0;
    px.bpred_trial( rate, distortion );
    const uint32_t cost = rdcost( P::mbmode_intra( C, B_PRED ) + rate, distortion, rate_mul, dist_mul );
    if ( cost < best_cost ) { best_cost = cost; best.mode = B_PRED; }
  }
  for ( int mode = TM_PRED; mode >= DC_PRED; mode-- ) {
    const uint32_t cost = rdcost( P::mbmode_intra( C, mode ), px.intra_variance( mode ), rate_mul, dist_mul );
    if ( cost < best_cost ) { best_cost = cost; best.mode = mode; }
  }
  // ---- inter, all from LAST: ZEROMV, NEARESTMV, NEARMV, NEWMV (a key frame has none) ----
  if constexpr ( !P::kKey ) {
    const ReencCosts & I = P::inter( C );
    const MvRefCosts ref_cost = mv_ref_costs( cen.probs, I.prob_cost );
    for ( int k = 0; k < 4; k++ ) {
      Mv mv;
      int mode = ZEROMV;
      uint32_t rate = ref_cost.zero;
      if ( k == 1 ) { mode = NEARESTMV; mv = cen.nearest; rate = ref_cost.nearest; }
      if ( k == 2 ) { mode = NEARMV; mv = cen.near; rate = ref_cost.near; }
      if ( k == 3 ) {
        mode = NEWMV;
        if ( I.quality == REENC_REALTIME && !( col % 4 == 0 && row % 4 == 0 ) ) continue;
        mv = newmv_search<P>( px, C, cen.best, col, row, mbw, mbh );
        rate = ref_cost.newmv + motion_vector_cost( I, mv.x - cen.best.x, mv.y - cen.best.y, 96 );
      }
      if ( k != 0 && mv.zero() ) continue;                       // the same as ZEROMV
      const uint32_t cost = rdcost( rate, px.inter_variance( mv.x, mv.y ), rate_mul, dist_mul );
      if ( cost < best_cost ) { best_cost = cost; best.mode = mode; best.mv = mv; }
    }
  }
  if ( best.mode <= B_PRED ) best.mv = Mv();
  return best;
}

// A job's ReencCosts (Costs::fill_mode_costs / fill_mv_component_costs, costs.cc:113-132,191-208), host only
inline void reenc_fill_costs( ReencCosts & C, const uint8_t mv_probs[2][19], int quality )
{
  std::memset( &C, 0, sizeof C );
  std::memcpy( C.prob_cost, k_prob_cost, sizeof C.prob_cost );
  for ( int a = 0; a < 10; a++ ) for ( int l = 0; l < 10; l++ ) tree_costs( C.bmode[a][l], k_kf_b_mode_probs + ( a * 10 + l ) * 9, kBModeTree, C.prob_cost );
  tree_costs( C.mbmode_intra, k_default_y_mode_probs, kYModeTree, C.prob_cost );
  for ( int comp = 0; comp < 2; comp++ ) {
    const uint8_t * p = mv_probs[comp];
    C.mv_comp[comp][0][0] = C.mv_comp[comp][1][0] = static_cast<uint16_t>( mv_component_cost( 0, p, C.prob_cost ) );
    for ( int i = 1; i <= 1023; i++ ) {
      const uint32_t c = mv_component_cost( static_cast<int16_t>( i ), p, C.prob_cost );
      C.mv_comp[comp][0][i] = static_cast<uint16_t>( c + C.prob_cost[p[1]] );
      C.mv_comp[comp][1][i] = static_cast<uint16_t>( c + C.prob_cost[255 - p[1]] );
    }
  }
  std::memcpy( C.mv_counts_to_probs, k_mv_counts_to_probs, 24 );
  C.quality = static_cast<uint8_t>( quality );
}

// Encoder::update_rd_multipliers (encoder.cc:178-193), in double as written there; y_ac: the quantiser's factor, not its index
inline void enc_rd_multipliers( uint16_t y_ac, uint32_t & rate_mul, uint32_t & dist_mul )
{
  const double q_ac = ( y_ac < 160 ) ? y_ac : 160.0;
  rate_mul = static_cast<uint32_t>( q_ac * q_ac * 2.80 );
  if ( rate_mul > 1000 ) { dist_mul = 1; rate_mul /= 100; }
  else dist_mul = 100;
}

// sad_per_bit16lut[q_index] (libvpx's table, encode_inter.cc:144-152): the values 2..14, each held for a run of indices
inline uint32_t enc_sad_per_bit( unsigned q_index )
{
  static constexpr uint8_t run[13] = { 16, 14, 12, 12, 12, 12, 12, 12, 8, 6, 6, 4, 2 };
  unsigned end = 0;
  for ( unsigned v = 0; v < 13; v++ ) { end += run[v]; if ( q_index < end ) return 2 + v; }
  return 14;
}

// Costs::fill_mv_sad_costs (costs.cc:135-149): the expression in float and double as written there, truncated
inline void enc_fill_mv_sad( uint16_t ( &mv_sad )[256] )
{
  mv_sad[0] = 300;
  for ( size_t i = 1; i <= 255; i++ ) {
    const size_t cost = 256 * ( 2 * log2f( 8 * i ) + 0.6 );
    mv_sad[i] = static_cast<uint16_t>( cost );
  }
}

// A forward inter job's cost block: the re-encode's (mbmode_costs[1], the stream's current vector probabilities) and what
// encode_raster<InterFrame> adds (encode_inter.cc:594-602)
inline void enc_fill_inter_costs( EncInterCosts & C, const uint8_t mv_probs[2][19], int quality, uint16_t y_ac, unsigned q_index )
{
  reenc_fill_costs( C.base, mv_probs, quality );
  enc_rd_multipliers( y_ac, C.rate_mul, C.dist_mul );
  C.sad_per_bit = enc_sad_per_bit( q_index );
  C.pad = 0;
  enc_fill_mv_sad( C.mv_sad );
}

// A key job's: the sub-block costs and mbmode_costs[0] (Costs::fill_mode_costs)
inline void enc_fill_key_costs( EncKeyCosts & C, uint16_t y_ac )
{
  std::memset( &C, 0, sizeof C );
  for ( int a = 0; a < 10; a++ ) for ( int l = 0; l < 10; l++ ) tree_costs( C.bmode[a][l], k_kf_b_mode_probs + ( a * 10 + l ) * 9, kBModeTree, k_prob_cost );
  tree_costs( C.mbmode, k_kf_y_mode_probs, kKfYModeTree, k_prob_cost );
  enc_rd_multipliers( y_ac, C.rate_mul, C.dist_mul );
}

} // namespace aa
