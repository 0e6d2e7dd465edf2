// The second pass's quantisation (aa_encode_two_pass_batch; Encoder::trellis_quantize and check_reset_y2, encoder.cc:198-408, run by
// encode_raster<KeyFrame> in its second pass, encode_intra.cc:409-439): a two-level ( q, q - 1 ) dynamic programme over a block's
// coefficients in zigzag order, from the last non-zero one down to the block type's first, under the token costs of the DEFAULT
// coefficient probabilities (the reference fills them from a fresh DecoderState, encode_intra.cc:395,414) and the job's multipliers.
// One source for k_encode_key2 (encode_two_pass_kernels.hip), its host simulation (tests/cpp/encode2_sim.cc) and the check against a plain
// array-of-nodes restatement (tests/cpp/trellis_check.cc); marked AA_MHD like vp8_math.hh.
//
// On the GPU the block's sixteen coefficients and the trellis live in registers: every loop over positions is fully unrolled and
// predicated on the coded length, so every index is a constant.  A node is one word (coefficient, token, next); of the rates and
// distortions only the two pairs of the position last built are alive.
#pragma once
#include <stdint.h>
#include <cstring>

#include "cost_tables.h"
#include "parse_common.hh"
#include "vp8_math.hh"
#include "vp8_tables.h"

namespace aa {

// BlockType (block.hh:44): the first index of the token cost table
enum : int { TQ_Y_AFTER_Y2 = 0, TQ_Y2 = 1, TQ_UV = 2, TQ_Y_WITHOUT_Y2 = 3 };
enum : uint32_t { TQ_ZERO = 0, TQ_ONE = 1, TQ_FOUR = 4, TQ_CAT1 = 5, TQ_CAT6 = 10, TQ_EOB = 11 };      // tokens.hh's token numbers

// What the trellis reads of the rate model: Costs::token_costs under the default probabilities, and the cost of a bool (for
// coeff_base_cost).  A constant; the runtime builds it once (trellis_fill_costs) and every job's cost block points at the one copy.
struct TrellisCosts {
  uint16_t token[4][8][3][12];      // [block type][band][context][token]
  uint16_t prob_cost[256];
};
static_assert( sizeof( TrellisCosts ) % 8 == 0, "TrellisCosts sits in a table of 8-byte aligned pieces" );

// vp8_coef_tree (costs.cc:38-51; RFC 6386 section 13.2): leaves are -token
constexpr int8_t kCoefTree[22] = { -11, 2, 0, 4, -1, 6, 8, 12, -2, 10, -3, -4, 14, 16, -5, -6, 18, 20, -7, -8, -9, -10 };

// Costs::compute_cost (costs.cc:151-170) from node `at`: uint16_t sums as there.  Host only.
inline void coef_tree_costs( uint16_t * costs, const uint8_t * probs, const uint16_t * prob_cost, int at, uint16_t sofar )
{
  for ( int i = 0; i < 2; i++ ) {
    const int entry = kCoefTree[at + i];
    const uint8_t p = probs[at / 2];
    const uint16_t c = static_cast<uint16_t>( sofar + prob_cost[i ? 255 - p : p] );
    if ( entry <= 0 ) costs[-entry] = c;
    else coef_tree_costs( costs, probs, prob_cost, entry, c );
  }
}

// Costs::fill_token_costs( default probabilities ) (costs.cc:172-189).  Where no end of block can stand -- context 0 beyond the block
// type's first band -- the tree is entered below its root and the end-of-block entry keeps the zero the reference's value-initialised
// Costs holds there (encoder.cc:77; the trellis does read it: a ZERO whose next node is an end of block).
inline void trellis_fill_costs( TrellisCosts & T )
{
  std::memset( &T, 0, sizeof T );
  std::memcpy( T.prob_cost, k_prob_cost, sizeof T.prob_cost );
  for ( int i = 0; i < 4; i++ )
    for ( int j = 0; j < 8; j++ )
      for ( int k = 0; k < 3; k++ )
        coef_tree_costs( T.token[i][j][k], k_default_coeff_probs + ( ( i * 8 + j ) * 3 + k ) * 11, T.prob_cost, ( k == 0 && j > ( i == 0 ? 1 : 0 ) ) ? 2 : 0, 0 );
}

// Costs::token_for_coeff (costs.cc:242-261)
AA_MHD uint32_t token_for_coeff( int coeff )
{
  const int a = coeff < 0 ? -coeff : coeff;
  return a <= 4 ? static_cast<uint32_t>( a ) : ( a <= 6 ? 5u : ( a <= 10 ? 6u : ( a <= 18 ? 7u : ( a <= 34 ? 8u : ( a <= 66 ? 9u : 10u ) ) ) ) );
}
AA_MHD uint32_t prev_token_class( uint32_t token ) { return token == TQ_ZERO || token == TQ_EOB ? 0u : ( token == TQ_ONE ? 1u : 2u ); }      // costs.hh:14

// Costs::coeff_base_cost (costs.cc:613-617) = libvpx's dct_value_cost, computed: what a coefficient costs beyond its token -- the
// extra bits of a value category under the category's fixed probabilities (RFC 6386 section 13.2: Pcat1 .. Pcat6, most significant bit
// first), and the sign, a bool of probability 128.  Zero costs nothing.  |coeff| <= 2048 + 66: eleven extra bits at the most.
AA_MHD uint32_t coeff_base_cost( int coeff, const uint16_t * prob_cost )
{
  if ( coeff == 0 ) return 0;
  const uint32_t a = static_cast<uint32_t>( coeff < 0 ? -coeff : coeff );
  uint32_t cost = prob_cost[coeff < 0 ? 255 - 128 : 128];
  if ( a <= 4 ) return cost;
  // the categories' bases, lengths and probabilities, a byte each, first bit lowest
  uint32_t base = 67, n = 11;
  uint64_t lo = 254ull | 254ull << 8 | 243ull << 16 | 230ull << 24 | 196ull << 32 | 177ull << 40 | 153ull << 48 | 140ull << 56, hi = 133ull | 130ull << 8 | 129ull << 16;
  if ( a <= 6 ) { base = 5; n = 1; lo = 159; }
  else if ( a <= 10 ) { base = 7; n = 2; lo = 165ull | 145ull << 8; }
  else if ( a <= 18 ) { base = 11; n = 3; lo = 173ull | 148ull << 8 | 140ull << 16; }
  else if ( a <= 34 ) { base = 19; n = 4; lo = 176ull | 155ull << 8 | 140ull << 16 | 135ull << 24; }
  else if ( a <= 66 ) { base = 35; n = 5; lo = 180ull | 157ull << 8 | 141ull << 16 | 134ull << 24 | 130ull << 32; }
  const uint32_t extra = a - base;
  for ( uint32_t i = 0; i < n; i++ ) {
    const uint32_t p = static_cast<uint32_t>( ( i < 8 ? lo >> ( 8 * i ) : hi >> ( 8 * ( i - 8 ) ) ) & 255u );
    cost += prob_cost[( ( extra >> ( n - 1 - i ) ) & 1u ) ? 255u - p : p];
  }
  return cost;
}

// Encoder::rdcost (encoder.cc:410-416), as reencode_search.hh's
AA_MHD uint32_t trellis_rdcost( uint32_t rate, uint32_t distortion, uint32_t rate_mul, uint32_t dist_mul ) { return ( ( 128u + rate * rate_mul ) / 256u ) + distortion * dist_mul; }

// Encoder::check_reset_y2 (encoder.cc:198-218), in front of the Y2 block's trellis: a Y2 block whose coefficients' magnitudes sum to
// less than 35 is dropped -- under the fine quantisers only, where a Y2 factor lies below 35
AA_MHD void check_reset_y2( int ( &c )[16], const int y2_dc, const int y2_ac )
{
  if ( y2_dc >= 35 && y2_ac >= 35 ) return;
  int sum = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
  for ( int i = 0; i < 16; i++ ) sum += c[i] < 0 ? -c[i] : c[i];
  if ( sum >= 35 ) return;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
  for ( int i = 0; i < 16; i++ ) c[i] = 0;
}

// A node of the trellis as one word: coefficient << 16 | token << 8 | next
AA_MHD uint32_t tq_node( int coeff, uint32_t token, uint32_t next ) { return ( static_cast<uint32_t>( coeff ) << 16 ) | ( token << 8 ) | next; }
AA_MHD int tq_coeff( uint32_t w ) { return static_cast<int>( w ) >> 16; }
AA_MHD uint32_t tq_token( uint32_t w ) { return ( w >> 8 ) & 255u; }
AA_MHD uint32_t tq_next( uint32_t w ) { return w & 255u; }

// What a walk found on its way, for the tests' census: nothing of it steers the encoder
struct TrellisTrace { bool ran, chose_lower; };

// Encoder::trellis_quantize (encoder.cc:220-408) in the three steps the kernel takes it in.  The dynamic programme reads nothing of
// the block's neighbours; the pick between its two entry nodes does, and what the walk from the picked node leaves is what the blocks
// to the right and below see as THEIR neighbour.  So sixteen lanes build sixteen trellises at once and only the picks are settled in
// block order (reencode_mb.hh).
//   build( c, .. )        c: the block's UNQUANTISED coefficients in raster order (int16_t values); type: TQ_*; fdc, fac: its factors
//   pick( ctx, .. )       -> the entry level under ctx = how many of the blocks above and to the left hold a coefficient (0..2)
//   nonzero_from( level ) -> whether the walk from that level would leave a coefficient
//   walk( c, level, .. )  c := the chosen quantised coefficients; -> whether one is left (Block::calculate_has_nonzero over all sixteen:
//                         under TQ_Y_AFTER_Y2 position 0 is not the trellis's and keeps what the caller left there, unless nothing from
//                         position 1 on was non-zero: then the reference clears the whole block)
struct Trellis {
  uint32_t w0[16], w1[16];          // the nodes of position k at the two levels; a position never built reads as the sentinel: an end of block
  uint32_t r0, r1, d0, d1, t0, t1;  // rate, distortion and token of the two nodes of the position built last (at first: the sentinel's)
  int first, coded;
  bool dc_kept;                     // position 0 lies in front of the trellis and holds a value

  AA_MHD void build( const int ( &c )[16], const int type, const int fdc, const int fac, const TrellisCosts & T, const uint32_t rate_mul, const uint32_t dist_mul )
  {
    first = type == TQ_Y_AFTER_Y2 ? 1 : 0;
    coded = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int k = 0; k < 16; k++ ) if ( k >= first && c[kZigzag[k]] != 0 ) coded = k + 1;
    dc_kept = first == 1 && coded != 0 && c[0] != 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int k = 0; k < 16; k++ ) w0[k] = w1[k] = tq_node( 0, TQ_EOB, 255 );
    r0 = r1 = d0 = d1 = 0; t0 = t1 = TQ_EOB;
    const uint16_t * costs = &T.token[type][0][0][0];
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int k = 15; k >= 0; k-- ) {
      if ( k >= coded || k < first ) continue;
      const int factor = k == 0 ? fdc : fac;
      const int original = static_cast<int16_t>( c[kZigzag[k]] );
      const int quantized = static_cast<int16_t>( original / factor );
      uint32_t nr[2], nd[2], nt[2], nw[2];
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
      for ( int level = 0; level < 2; level++ ) {
        int candidate = quantized;
        if ( candidate < 0 ) { candidate += level; candidate = candidate > 0 ? 0 : candidate; }
        else if ( candidate > 0 || level == 0 ) { candidate -= level; candidate = candidate < 0 ? 0 : candidate; }
        else { nr[1] = nr[0]; nd[1] = nd[0]; nt[1] = nt[0]; nw[1] = nw[0]; continue; }      // zero has no level below it: the other node's copy
        const int diff = static_cast<int16_t>( original - candidate * factor );         // (int16_t as there, before it is squared)
        const uint32_t sse = static_cast<uint32_t>( diff * diff );
        const uint32_t token = token_for_coeff( candidate );
        // the rate of the NEXT token under THIS token's context
        uint32_t rate0 = r0, rate1 = r1;
        if ( k < 15 ) {
          const uint16_t * row = costs + ( kBand[k + 1] * 3 + prev_token_class( token ) ) * 12;
          rate0 += row[t0]; rate1 += row[t1];
        }
        const uint32_t dist0 = d0 + sse, dist1 = d1 + sse;
        const uint32_t best = trellis_rdcost( rate1, dist1, rate_mul, dist_mul ) < trellis_rdcost( rate0, dist0, rate_mul, dist_mul ) ? 1u : 0u;
        if ( candidate != 0 || ( best ? t1 : t0 ) != TQ_EOB ) {
          nr[level] = ( best ? rate1 : rate0 ) + coeff_base_cost( candidate, T.prob_cost );
          nd[level] = best ? dist1 : dist0;
          nt[level] = token;
          nw[level] = tq_node( candidate, token, best );
        } else {                                         // a zero in front of the end of block: the end of block moves back here
          nr[level] = 0; nd[level] = sse; nt[level] = TQ_EOB;
          nw[level] = tq_node( 0, TQ_EOB, 255 );
        }
      }
      r0 = nr[0]; r1 = nr[1]; d0 = nd[0]; d1 = nd[1]; t0 = nt[0]; t1 = nt[1];
      w0[k] = nw[0]; w1[k] = nw[1];
    }
  }

  // the first token's own rate, under the neighbours' context, decides between the two entry nodes
  AA_MHD uint32_t pick( const uint32_t ctx, const int type, const TrellisCosts & T, const uint32_t rate_mul, const uint32_t dist_mul ) const
  {
    const uint16_t * row = &T.token[type][kBand[first]][ctx][0];
    return trellis_rdcost( r1 + row[t1], d1, rate_mul, dist_mul ) < trellis_rdcost( r0 + row[t0], d0, rate_mul, dist_mul ) ? 1u : 0u;
  }

  AA_MHD bool nonzero_from( uint32_t level ) const
  {
    bool done = false, any = dc_kept;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int k = 0; k < 16; k++ ) {
      const uint32_t w = level ? w1[k] : w0[k];
      if ( k < first || done || tq_token( w ) == TQ_EOB ) { done |= k >= first; continue; }
      any |= tq_coeff( w ) != 0;
      level = tq_next( w );
    }
    return any;
  }

  // the walk along `next`, up to the end of block; everything behind it is zero
  AA_MHD bool walk( int ( &c )[16], uint32_t level, const int fdc, const int fac, TrellisTrace * trace = nullptr ) const
  {
    bool done = false, any = dc_kept, lower = false;
    if ( first == 1 && coded == 0 ) c[0] = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int k = 0; k < 16; k++ ) {
      if ( k < first ) continue;
      const uint32_t w = level ? w1[k] : w0[k];
      const int truncated = static_cast<int16_t>( static_cast<int16_t>( c[kZigzag[k]] ) / ( k == 0 ? fdc : fac ) );
      if ( done || tq_token( w ) == TQ_EOB ) { done = true; lower |= truncated != 0; c[kZigzag[k]] = 0; continue; }
      lower |= tq_coeff( w ) != truncated;
      c[kZigzag[k]] = tq_coeff( w );
      any |= tq_coeff( w ) != 0;
      level = tq_next( w );
    }
    if ( trace ) { trace->ran = coded != 0; trace->chose_lower = lower; }
    return any;
  }
};

// the three steps in one: a block whose neighbours are settled
AA_MHD bool trellis_quantize( int ( &c )[16], const int type, const int fdc, const int fac, const uint32_t ctx, const TrellisCosts & T, const uint32_t rate_mul,
                              const uint32_t dist_mul, TrellisTrace * trace = nullptr )
{
  Trellis t;
  t.build( c, type, fdc, fac, T, rate_mul, dist_mul );
  return t.walk( c, t.pick( ctx, type, T, rate_mul, dist_mul ), fdc, fac, trace );
}

} // namespace aa
