// What the FIRST pass of a two-pass key frame leaves behind for the second (aa_encode_two_pass_batch; encode_raster<KeyFrame> with
// two_pass_encoder_, encode_intra.cc:409-439), read off the first pass's raw output -- the records, masks and dense slots k_encode_key
// leaves, before any host has finished them:
//   first_pass_bits     a macroblock's two side bits (reencode_search.hh, EncKey2Costs)
//   count_raw_block     accumulate_token_branches for one block of that output, as k_token_counts counts a finished frame's
//                       (serialize_common.hh): the first pass's branch counts make its token_prob_update, and the reference never
//                       clears that field between the passes (optimize_probability_tables only writes where its own probability is
//                       above zero and not the default's, encoder.cc:432-434)
//   merge_update        the field both passes leave: the second pass's update where it makes one, else the first pass's
// One source for k_key2_first_pass / k_key2_updates (encode_two_pass_kernels.hip) and the host simulation (tests/cpp/encode2_sim.cc).
#pragma once
#include "serialize_common.hh"

namespace aa {

// the mask a macroblock's blocks and its neighbours read: a B_PRED macroblock has no Y2 block whatever bit 24 says
AA_BW_HD uint32_t raw_context_mask( const aa_mb_info & rec, const uint32_t mask ) { return rec.y_mode == B_PRED ? mask & 0xFFFFFFu : mask; }

AA_BW_HD uint8_t first_pass_bits( const aa_mb_info & rec, const uint32_t mask )
{
  return static_cast<uint8_t>( ( rec.y_mode == B_PRED ? 1u : 0u ) | ( ( ( raw_context_mask( rec, mask ) >> 24 ) & 1u ) << 1 ) );
}

// block b = 0..23 of macroblock mi (Y2 blocks are not counted: serializer.cc:582-586); dense: [mbw * mbh][25][16]
template <class A> AA_BW_HD void count_raw_block( A add, const aa_mb_info * recs, const uint32_t * masks, const int16_t * dense, const uint32_t mbw, const uint32_t mi, const uint32_t b )
{
  const uint32_t col = mi % mbw, row = mi / mbw;
  const uint32_t nz = raw_context_mask( recs[mi], masks[mi] );
  const uint32_t above = row ? raw_context_mask( recs[mi - mbw], masks[mi - mbw] ) : 0u, left = col ? raw_context_mask( recs[mi - 1], masks[mi - 1] ) : 0u;
  const bool has_y2 = recs[mi].y_mode != B_PRED;
  const int16_t * v = dense + ( static_cast<size_t>( mi ) * 25 + b ) * 16;
  uint32_t zmask = 0;
  if ( ( nz >> b ) & 1u ) for ( uint32_t j = 0; j < 16; j++ ) if ( v[j] ) zmask |= 1u << ( static_cast<uint32_t>( ser::kInvZigzagNib >> ( 4 * j ) ) & 15u );
  const uint32_t type = b >= 16 ? 2u : ( has_y2 ? 0u : 3u ), first = ( b < 16 && has_y2 ) ? 1u : 0u;
  ser::count_block( add, type, first, ser::block_context( b, nz, above, left ), zmask, [=]( const uint32_t k ) { return static_cast<int>( v[ser::zigzag( k )] ); } );
}

// optimize_probability_tables for one field of a key frame: counts -> ( flag, value ) against the default table
AA_BW_HD void key_update( const uint32_t false_count, const uint32_t true_count, const uint8_t current, uint8_t & flag, uint8_t & value )
{
  const uint32_t prob = ser::calc_prob( false_count, false_count + true_count );
  flag = prob > 0 && prob != current;
  value = flag ? static_cast<uint8_t>( prob ) : 0;
}

AA_BW_HD void merge_update( uint8_t & flag, uint8_t & value, const uint8_t first_flag, const uint8_t first_value )
{
  if ( !flag && first_flag ) { flag = 1; value = first_value; }
}

} // namespace aa
