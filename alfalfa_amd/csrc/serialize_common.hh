// Token serialisation shared by the device (serialize_kernels.hip: k_serialize_tokens, a lane per job and DCT partition) and the host
// (serializer.cpp; tests/cpp/bool_writer_check.cc): Block::serialize_tokens and Macroblock::serialize_tokens (serializer.cc:429-443,
// 595-739) over the RECORDS -- aa_mb_info + coefficient blocks, dense or packed (coeff_pack.hh) -- instead of the reference's Frame.
//
// Nothing here is carried from macroblock to macroblock but one bit: a block's above / left context is the nz_mask bit of the block
// above / to the left, in the macroblock itself or in the neighbour's record (a skipped macroblock has an empty mask: its contexts are
// cleared, macroblock.cc:475-502), so partition p's lane never needs what partition p - 1's lane is doing to the row above.  The one
// exception is the Y2 chain (relink_y2_blocks, frame.cc:255-269): a Y2 block's neighbours are the last macroblocks of its column / row
// that HAVE a Y2 block -- to the left a bit the lane carries along its row, above a walk up the column's records (usually one step).
// No arrays are indexed with run-time values: a lane keeps everything in registers (tests/test_serialize_kernel_resources.py).
#pragma once
#include <stdint.h>

#include "../../include/alfalfa_amd.h"
#include "bool_writer.hh"
#include "parse_common.hh"

namespace aa {
namespace ser {

// (4 bits per position: parse_common.hh's kZigzag / kBand, as constants a lane shifts)
constexpr uint64_t kZigzagNib = 0xFEB7ADC9'63258410ull;   // zigzag position k -> raster position { 0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15 }
constexpr uint64_t kInvZigzagNib = 0xFEA9DB83'C7426510ull; // raster position j -> zigzag position { 0, 1, 5, 6, 2, 4, 7, 12, 3, 8, 11, 13, 9, 10, 14, 15 }
constexpr uint64_t kBandNib = 0x76666666'65463210ull;    // zigzag position k -> band { 0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7 } (position 16: band 0 is never read)
constexpr bool nibbles_ok()
{
  for ( unsigned k = 0; k < 16; k++ )
    if ( ( ( kZigzagNib >> ( 4 * k ) ) & 15u ) != kZigzag[k] || ( ( kBandNib >> ( 4 * k ) ) & 15u ) != kBand[k] || ( ( kInvZigzagNib >> ( 4 * kZigzag[k] ) ) & 15u ) != k ) return false;
  return true;
}
static_assert( nibbles_ok(), "the nibble tables are not parse_common.hh's kZigzag / kBand" );
AA_BW_HD uint32_t zigzag( uint32_t k ) { return static_cast<uint32_t>( kZigzagNib >> ( 4 * k ) ) & 15u; }
AA_BW_HD uint32_t band( uint32_t k ) { return static_cast<uint32_t>( kBandNib >> ( 4 * k ) ) & 15u; }
AA_BW_HD uint32_t popc( uint32_t v ) { return static_cast<uint32_t>( __builtin_popcount( v ) ); }

// extra-bit probabilities of the DCT value categories 3..6 (tokens.cc: token_decoder_2 .. token_decoder_5), a byte each, first bit lowest
constexpr uint64_t kCat3 = 173ull | 148ull << 8 | 140ull << 16;
constexpr uint64_t kCat4 = 176ull | 155ull << 8 | 140ull << 16 | 135ull << 24;
constexpr uint64_t kCat5 = 180ull | 157ull << 8 | 141ull << 16 | 134ull << 24 | 130ull << 32;
constexpr uint64_t kCat6Lo = 254ull | 254ull << 8 | 243ull << 16 | 230ull << 24 | 196ull << 32 | 177ull << 40 | 153ull << 48 | 140ull << 56;
constexpr uint64_t kCat6Hi = 133ull | 130ull << 8 | 129ull << 16;

// TokenDecoder<n>::encode: n bits of `inc`, most significant first
template <class W> AA_BW_HD void put_extra( W & w, const uint32_t inc, const int n, const uint64_t lo, const uint64_t hi )
{
  for ( int i = 0; i < n; i++ ) {
    const uint32_t p = static_cast<uint32_t>( ( i < 8 ? lo >> ( 8 * i ) : hi >> ( 8 * ( i - 8 ) ) ) & 255u );
    w.put( ( inc >> ( n - 1 - i ) ) & 1u, p );
  }
}

// Block::serialize_tokens.  probs: the block type's [8][3][11] table; first: 1 for a Y block beside a Y2 block; ctx: coded neighbours
// (0..2); zmask: bit k = zigzag position k holds a coefficient; value( k ): that coefficient.
template <class W, class V> AA_BW_HD void write_block( W & w, const uint8_t * probs, const uint32_t first, uint32_t ctx, uint32_t zmask, V value )
{
  zmask &= first ? 0xFFFEu : 0xFFFFu;
  const uint32_t coded = zmask ? 32u - static_cast<uint32_t>( __builtin_clz( zmask ) ) : 0u;
  bool last_was_zero = false;
  uint32_t k = first;
  for ( ; k < coded; k++ ) {
    const uint8_t * p = probs + ( band( k ) * 3u + ctx ) * 11u;
    if ( !last_was_zero ) w.put( 1, p[0] );
    if ( !( ( zmask >> k ) & 1u ) ) { w.put( 0, p[1] ); last_was_zero = true; ctx = 0; continue; }
    const int c = value( k );
    const uint32_t v = static_cast<uint32_t>( c < 0 ? -c : c );
    last_was_zero = false;
    w.put( 1, p[1] );
    if ( v == 1 ) { w.put( 0, p[2] ); ctx = 1; }
    else {
      ctx = 2;
      w.put( 1, p[2] );
      if ( v <= 4 ) {
        w.put( 0, p[3] );
        if ( v == 2 ) w.put( 0, p[4] );
        else { w.put( 1, p[4] ); w.put( v == 4, p[5] ); }
      } else {
        w.put( 1, p[3] );
        if ( v <= 10 ) {
          w.put( 0, p[6] );
          if ( v <= 6 ) { w.put( 0, p[7] ); w.put( v == 6, 159 ); }
          else { w.put( 1, p[7] ); w.put( ( ( v - 7 ) >> 1 ) & 1u, 165 ); w.put( ( v - 7 ) & 1u, 145 ); }
        } else {
          w.put( 1, p[6] );
          if ( v <= 34 ) {
            w.put( 0, p[8] );
            if ( v <= 18 ) { w.put( 0, p[9] ); put_extra( w, v - 11, 3, kCat3, 0 ); }
            else { w.put( 1, p[9] ); put_extra( w, v - 19, 4, kCat4, 0 ); }
          } else {
            w.put( 1, p[8] );
            if ( v <= 66 ) { w.put( 0, p[10] ); put_extra( w, v - 35, 5, kCat5, 0 ); }
            else { w.put( 1, p[10] ); put_extra( w, ( v - 67 ) & 0x7FFu, 11, kCat6Lo, kCat6Hi ); }   // (the reference refuses values above 2114; a parse never produces one)
          }
        }
      }
    }
    w.put( c < 0 );
  }
  if ( coded < 16 ) w.put( 0, probs[( band( k ) * 3u + ctx ) * 11u] );       // end of block
}

// accumulate_token_branches (serializer.cc:456-579) for one block: the branches write_block takes, counted instead of written.
// add( node, taken ): one more `taken` (0 false, 1 true) at node 0..1055 = ( ( type * 8 + band ) * 3 + context ) * 11 + tree node.
template <class A, class V> AA_BW_HD void count_block( A add, const uint32_t type, const uint32_t first, uint32_t ctx, uint32_t zmask, V value )
{
  zmask &= first ? 0xFFFEu : 0xFFFFu;
  const uint32_t coded = zmask ? 32u - static_cast<uint32_t>( __builtin_clz( zmask ) ) : 0u;
  bool last_was_zero = false;
  uint32_t k = first;
  for ( ; k < coded; k++ ) {
    const uint32_t at = ( ( type * 8u + band( k ) ) * 3u + ctx ) * 11u;
    if ( !last_was_zero ) add( at, 1u );
    if ( !( ( zmask >> k ) & 1u ) ) { add( at + 1, 0u ); last_was_zero = true; ctx = 0; continue; }
    const int c = value( k );
    const uint32_t v = static_cast<uint32_t>( c < 0 ? -c : c );
    last_was_zero = false;
    add( at + 1, 1u );
    if ( v == 1 ) { add( at + 2, 0u ); ctx = 1; continue; }
    ctx = 2;
    add( at + 2, 1u );
    if ( v <= 4 ) {
      add( at + 3, 0u );
      if ( v == 2 ) add( at + 4, 0u );
      else { add( at + 4, 1u ); add( at + 5, v == 4 ? 1u : 0u ); }
    } else {
      add( at + 3, 1u );
      if ( v <= 10 ) { add( at + 6, 0u ); add( at + 7, v <= 6 ? 0u : 1u ); }
      else {
        add( at + 6, 1u );
        if ( v <= 34 ) { add( at + 8, 0u ); add( at + 9, v <= 18 ? 0u : 1u ); }
        else { add( at + 8, 1u ); add( at + 10, v <= 66 ? 0u : 1u ); }
      }
    }
  }
  if ( coded < 16 ) add( ( ( type * 8u + band( k ) ) * 3u + ctx ) * 11u, 0u );       // end of block
}

// Encoder::calc_prob (encoder.cc:48-55), exactly: 0 when nothing was false, else 256 * false / total clamped to 1..255
AA_BW_HD uint32_t calc_prob( const uint32_t false_count, const uint32_t total )
{
  if ( !false_count ) return 0;
  const uint32_t p = static_cast<uint32_t>( 256ull * false_count / total );
  return p < 1 ? 1 : ( p > 255 ? 255 : p );
}

// a block's coded neighbours (0..2): b = 0..15 Y, 16..19 U, 20..23 V; nz = the macroblock's own mask, above / left = the neighbours'
AA_BW_HD uint32_t block_context( const uint32_t b, const uint32_t nz, const uint32_t above, const uint32_t left )
{
  if ( b < 16 ) {
    const uint32_t a = b >= 4 ? ( nz >> ( b - 4 ) ) & 1u : ( above >> ( 12 + b ) ) & 1u;
    const uint32_t l = ( b & 3 ) ? ( nz >> ( b - 1 ) ) & 1u : ( left >> ( b + 3 ) ) & 1u;
    return a + l;
  }
  const uint32_t k = ( b - 16 ) & 3u;
  const uint32_t a = k >= 2 ? ( nz >> ( b - 2 ) ) & 1u : ( above >> ( b + 2 ) ) & 1u;
  const uint32_t l = ( k & 1 ) ? ( nz >> ( b - 1 ) ) & 1u : ( left >> ( b + 1 ) ) & 1u;
  return a + l;
}

// the mask a neighbour hands on: a skipped macroblock's contexts are cleared (its mask is empty; so is that of a macroblock flagged
// AA_MB_SKIP in a frame whose header has no prob_skip_false -- there the flag cannot be said and the empty blocks are written)
AA_BW_HD uint32_t context_mask( const aa_mb_info & mb ) { return ( mb.flags & AA_MB_SKIP ) ? 0u : mb.nz_mask; }

// Macroblock::serialize_tokens for macroblock (col, row).  coeffs / packed: aa_dev_frame's -- dense: 16-coefficient blocks in raster order,
// the macroblock's at coeff_index, stored blocks in parse order; packed: the heap's base, the macroblock's words at reserved << 32 |
// coeff_index (coeff_pack.hh).  left_y2: the Y2 chain's bit along this row (0 at the row's start), updated.
template <class W> AA_BW_HD void write_macroblock( W & w, const uint8_t * probs, const aa_mb_info * mbs, const uint32_t mbw, const uint32_t col, const uint32_t row,
                                                   const int16_t * coeffs, const bool packed, const bool skip_enabled, uint32_t & left_y2 )
{
  const size_t mi = static_cast<size_t>( row ) * mbw + col;
  const aa_mb_info & mb = mbs[mi];
  const bool has_y2 = mb.flags & AA_MB_HAS_Y2;
  if ( skip_enabled && ( mb.flags & AA_MB_SKIP ) ) { if ( has_y2 ) left_y2 = 0; return; }
  const uint32_t nz = context_mask( mb );
  const uint32_t above = row ? context_mask( mbs[mi - mbw] ) : 0u, left = col ? context_mask( mbs[mi - 1] ) : 0u;
  const int16_t * at = packed ? coeffs + ( static_cast<size_t>( mb.reserved ) << 32 | mb.coeff_index ) : coeffs + static_cast<size_t>( mb.coeff_index ) * 16;
  const int16_t * const slots = at;          // packed: the 25 mask slots
  if ( packed ) at += 25;
  const uint32_t ytype = has_y2 ? 0u : 3u, yfirst = has_y2 ? 1u : 0u;

  for ( uint32_t p = has_y2 ? 0u : 1u; p < 25; p++ ) {   // parse order: Y2, Y 0..15, U 16..19, V 20..23 (one body: everything inlines into it)
    const uint32_t b = p ? p - 1u : 24u;
    uint32_t type, first = 0, ctx;
    if ( b == 24 ) {
      uint32_t above_y2 = 0;
      for ( uint32_t r = row; r-- > 0; ) {               // the last macroblock above that has a Y2 block
        const aa_mb_info & nb = mbs[static_cast<size_t>( r ) * mbw + col];
        if ( nb.flags & AA_MB_HAS_Y2 ) { above_y2 = ( context_mask( nb ) >> 24 ) & 1u; break; }
      }
      type = 1; ctx = above_y2 + left_y2;
      left_y2 = ( nz >> 24 ) & 1u;
    } else if ( b < 16 ) {
      const uint32_t a = b >= 4 ? ( nz >> ( b - 4 ) ) & 1u : ( above >> ( 12 + b ) ) & 1u;
      const uint32_t l = ( b & 3 ) ? ( nz >> ( b - 1 ) ) & 1u : ( left >> ( b + 3 ) ) & 1u;
      type = ytype; first = yfirst; ctx = a + l;
    } else {                                             // U 16..19, V 20..23: 2 x 2 each
      const uint32_t k = ( b - 16 ) & 3u;
      const uint32_t a = k >= 2 ? ( nz >> ( b - 2 ) ) & 1u : ( above >> ( b + 2 ) ) & 1u;
      const uint32_t l = ( k & 1 ) ? ( nz >> ( b - 1 ) ) & 1u : ( left >> ( b + 1 ) ) & 1u;
      type = 2; ctx = a + l;
    }
    uint32_t zmask = 0;
    const int16_t * const v = at;
    if ( ( nz >> b ) & 1u ) {                            // stored: `at` moves past it
      if ( packed ) { zmask = static_cast<uint16_t>( slots[b] ); at += popc( zmask ); }
      else {
        for ( uint32_t j = 0; j < 16; j++ ) if ( v[j] ) zmask |= 1u << ( static_cast<uint32_t>( kInvZigzagNib >> ( 4 * j ) ) & 15u );
        at += 16;
      }
    }
    write_block( w, probs + type * ( 8 * 3 * 11 ), first, ctx, zmask,
                 [=]( const uint32_t k ) { return static_cast<int>( packed ? v[popc( zmask & ( ( 1u << k ) - 1u ) )] : v[zigzag( k )] ); } );
  }
}

// DCT partition `part` of `nparts`: macroblock rows row % nparts == part in raster order, then BoolEncoder::finish -> the bytes it takes
template <class W> AA_BW_HD uint32_t write_partition( W & w, const uint8_t * probs, const aa_mb_info * mbs, const uint32_t mbw, const uint32_t mbh,
                                                      const int16_t * coeffs, const bool packed, const bool skip_enabled, const uint32_t part, const uint32_t nparts )
{
  for ( uint32_t row = part; row < mbh; row += nparts ) {
    uint32_t left_y2 = 0;
    for ( uint32_t col = 0; col < mbw; col++ ) write_macroblock( w, probs, mbs, mbw, col, row, coeffs, packed, skip_enabled, left_y2 );
  }
  return w.finish();
}

} // namespace ser
} // namespace aa
