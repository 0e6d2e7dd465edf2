// The size of an estimate's frame (aa_estimate_size_batch; Encoder::estimate_size, size_estimation.cc:88-95,163-170), host and device (one
// source): Frame::serialize's DCT partition -- the small frame has one -- walked with serialize_common.hh's block writer straight over what
// the decision kernels leave (the records' modes, the raw masks, the dense 25-slot coefficients), without the compaction a frame that is
// kept goes through.  Given a BoolWriter of no capacity the walk stores nothing and counts: finish() is the partition's size.  What
// optimize_prob_skip and optimize_interframe_probs count falls out of the same walk.
#pragma once
#include <stdint.h>

#include "serialize_common.hh"

namespace aa {
namespace est {

// what the serialiser would find in the finished record of a macroblock the decision left as (y_mode, raw mask): rebase_records' rule
AA_BW_HD bool has_y2( const aa_mb_info & mb ) { return mb.y_mode != B_PRED && mb.y_mode != SPLITMV; }
AA_BW_HD uint32_t coded_mask( const aa_mb_info & mb, const uint32_t raw ) { return raw & ( has_y2( mb ) ? 0x1FFFFFFu : 0xFFFFFFu ); }

struct Counts { uint32_t token_bytes, with_coefficients, intra, pad; };

// Macroblock::serialize_tokens over every macroblock in raster order, then BoolEncoder::finish.  recs: y_mode and ref_frame are read;
// masks: the decision's raw masks; dense: [mbw * mbh][25][16].  A macroblock without a coefficient is skipped (the estimate's header
// always has prob_skip_false) and hands on empty contexts, as serialize_common.hh's write_macroblock has it.
template <class W> AA_BW_HD Counts write_tokens( W & w, const uint8_t * probs, const aa_mb_info * recs, const uint32_t * masks, const int16_t * dense, const uint32_t mbw,
                                                 const uint32_t mbh )
{
  Counts c;
  c.token_bytes = 0; c.with_coefficients = 0; c.intra = 0; c.pad = 0;
  uint64_t y2a0 = 0, y2a1 = 0, y2a2 = 0, y2a3 = 0, above_bits_before = 0;
  for ( uint32_t row = 0; row < mbh; row++ ) {
    uint32_t left_y2 = 0;
    for ( uint32_t col = 0; col < mbw; col++ ) {
      const size_t mi = static_cast<size_t>( row ) * mbw + col;
      const aa_mb_info & mb = recs[mi];
      const bool y2 = has_y2( mb );
      const uint32_t nz = coded_mask( mb, masks[mi] );
      if ( mb.ref_frame == 0 ) c.intra++;
      // the Y2 chain upwards (relink_y2_blocks): per column the Y2 bit of the last macroblock that has a Y2 block, a bit each in four words
      // named one by one (an array indexed at run time would go to private memory); a small frame wider than 256 macroblocks walks up instead
      if ( y2 ) {
        const uint64_t bit = 1ull << ( col & 63u ), on = ( nz >> 24 ) & 1u ? bit : 0ull;
        const uint64_t w0 = y2a0, w1 = y2a1, w2 = y2a2, w3 = y2a3;
        above_bits_before = col < 64 ? w0 : ( col < 128 ? w1 : ( col < 192 ? w2 : w3 ) );
        y2a0 = col < 64 ? ( w0 & ~bit ) | on : w0; y2a1 = col >= 64 && col < 128 ? ( w1 & ~bit ) | on : w1;
        y2a2 = col >= 128 && col < 192 ? ( w2 & ~bit ) | on : w2; y2a3 = col >= 192 ? ( w3 & ~bit ) | on : w3;
      }
      if ( !nz ) { if ( y2 ) left_y2 = 0; continue; }
      c.with_coefficients++;
      const uint32_t above = row ? coded_mask( recs[mi - mbw], masks[mi - mbw] ) : 0u, left = col ? coded_mask( recs[mi - 1], masks[mi - 1] ) : 0u;
      const int16_t * const slots = dense + mi * 25 * 16;
      for ( uint32_t p = y2 ? 0u : 1u; p < 25; p++ ) {                 // parse order: Y2, Y 0..15, U 16..19, V 20..23
        const uint32_t b = p ? p - 1u : 24u;
        uint32_t type, first = 0, ctx;
        if ( b == 24 ) {
          uint32_t above_y2;
          if ( mbw <= 256 ) above_y2 = static_cast<uint32_t>( ( above_bits_before >> ( col & 63u ) ) & 1u );
          else {
            above_y2 = 0;
            for ( uint32_t r = row; r-- > 0; ) {                        // the last macroblock above that has a Y2 block
              const size_t ni = static_cast<size_t>( r ) * mbw + col;
              if ( has_y2( recs[ni] ) ) { above_y2 = ( coded_mask( recs[ni], masks[ni] ) >> 24 ) & 1u; break; }
            }
          }
          type = 1; ctx = above_y2 + left_y2;
          left_y2 = ( nz >> 24 ) & 1u;
        } else {
          type = b < 16 ? ( y2 ? 0u : 3u ) : 2u; first = ( b < 16 && y2 ) ? 1u : 0u;
          ctx = ser::block_context( b, nz, above, left );
        }
        uint32_t zmask = 0;
        const int16_t * const v = slots + b * 16;
        if ( ( nz >> b ) & 1u )
          for ( uint32_t j = 0; j < 16; j++ ) if ( v[j] ) zmask |= 1u << ( static_cast<uint32_t>( ser::kInvZigzagNib >> ( 4 * j ) ) & 15u );
        ser::write_block( w, probs + type * ( 8 * 3 * 11 ), first, ctx, zmask, [=]( const uint32_t k ) { return static_cast<int>( v[ser::zigzag( k )] ); } );
      }
    }
  }
  c.token_bytes = w.finish();
  return c;
}

} // namespace est
} // namespace aa
