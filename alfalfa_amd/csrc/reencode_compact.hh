// What a re-encoded frame's records need beyond the compaction rule of rebase_compact.hh, one source for host and device: the re-encode
// decides every mode on the device, so what aa_rebase_device_batch reads off its input records on the host -- the intra-row words, the
// intra count, the intra diagonals -- and the per-macroblock loop-filter level that reencode_records (runtime_reencode.inc) sets are
// stated here as pure functions.  k_reencode_count / k_reencode_compact (reencode_compact_kernels.hip), aa_reencode_device_batch and
// tests/cpp/reencode_compact_check.cc compile the same text.
#pragma once
#include <stdint.h>

#include "parse_common.hh"      // HeaderParams, mb_lf_level
#include "rebase_compact.hh"

namespace aa {
namespace compact {

// ---- the intra-row words: bit col & 63 of word row * words_per_row + col / 64 is set where macroblock (col, row) is intra ----
AA_MHD uint32_t words_per_row( const uint32_t mbw ) { return ( mbw + 63 ) / 64; }
AA_MHD uint32_t row_words( const uint32_t mbw, const uint32_t mbh ) { return words_per_row( mbw ) * mbh; }      // (never more than mbw * mbh: a word per macroblock would do)

// word w of a frame, from the records the decision wrote: its (at most 64) macroblocks' ref_frame, nothing else
AA_MHD unsigned long long intra_row_word( const aa_mb_info * mbs, const uint32_t mbw, const uint32_t w )
{
  const uint32_t per_row = words_per_row( mbw ), row = w / per_row, col0 = ( w - row * per_row ) * 64;
  const uint32_t cols = mbw - col0 < 64 ? mbw - col0 : 64;
  const aa_mb_info * at = mbs + static_cast<size_t>( row ) * mbw + col0;
  unsigned long long bits = 0;
  for ( uint32_t c = 0; c < cols; c++ ) if ( at[c].ref_frame == 0 ) bits |= 1ull << c;
  return bits;
}

// ---- what the host derives from the words once they are down ----
AA_MHD uint32_t intra_count( const unsigned long long * rows, const uint32_t words )
{
  uint32_t n = 0;
  for ( uint32_t w = 0; w < words; w++ ) n += static_cast<uint32_t>( __builtin_popcountll( rows[w] ) );
  return n;
}
// diagonals[col + 2 * row] = 1 where macroblock (col, row) is intra; diagonals: mbw + 2 * (mbh - 1) bytes, zeroed by the caller
AA_MHD void intra_diagonals( const unsigned long long * rows, const uint32_t mbw, const uint32_t mbh, uint8_t * diagonals )
{
  const uint32_t per_row = words_per_row( mbw );
  for ( uint32_t row = 0; row < mbh; row++ )
    for ( uint32_t col = 0; col < mbw; col++ )
      if ( ( rows[row * per_row + ( col >> 6 )] >> ( col & 63 ) ) & 1ull ) diagonals[col + 2 * row] = 1;
}

// ---- the loop-filter level ----
// What mb_lf_level reads of a re-encoded frame: the new header's level for every segment, and the stream's current filter adjustments
// where both the header and the stream have them switched on.  Everything else stays zero.
AA_MHD void lf_params( HeaderParams & fp, const uint8_t loop_filter_level, const bool adjustments, const int8_t * ref, const int8_t * mode )
{
  fp = HeaderParams();
  fp.loop_filter_level = loop_filter_level;
  for ( int g = 0; g < 4; g++ ) fp.seg_level[g] = loop_filter_level;
  if ( adjustments ) {
    fp.fadj_enabled = 1;
    for ( int k = 0; k < 4; k++ ) { fp.fadj_ref[k] = ref[k]; fp.fadj_mode[k] = mode[k]; }
  }
}

// the output record of a re-encoded macroblock: the rebase's (flags, nz_mask, coeff_index) with lf_level added; segment_id is the
// decision's 0
AA_MHD aa_mb_info reencode_record( const aa_mb_info & in, const uint32_t raw_mask, const uint32_t coeff_index, const HeaderParams & fp )
{
  aa_mb_info m = output_record( in, raw_mask, coeff_index );
  m.lf_level = mb_lf_level( fp, 0, m.ref_frame, m.y_mode );
  return m;
}

} // namespace compact
} // namespace aa
