// The rule of the loop-filter level search, host and device (one source): Encoder::apply_best_loopfilter_settings' choice
// (encoder.cc:489-503) -- levels in ascending order from level_lo, a candidate replaces the best only if its score is GREATER, the first
// one that does not ends the search -- continued over ROUNDS of consecutive levels, so that a search scored K levels at a time
// (aa_lf_search_decode_batch: k_lf_choose, a thread per job; its state lives in device memory between rounds) ends exactly where the plain
// loop over all scores (choose_level, runtime_lf_search.inc) ends.  And the per-segment level a macroblock record gets for a header
// level (segment_levels there), which k_lf_candidates and k_lf_finish apply on the device.
#pragma once
#include <stdint.h>

#if defined( __HIPCC__ )
#define AA_LFC_HD __host__ __device__ inline __attribute__( ( always_inline ) )
#else
#define AA_LFC_HD inline
#endif

namespace aa {

// A search between rounds.  evaluated: candidates the rule has consumed -- every one that improved and the one that did not.
struct LfChoice {
  int32_t best_level;
  int32_t evaluated;
  int32_t done;
  int32_t pad;
  double best_score;
};

AA_LFC_HD void lf_choice_begin( LfChoice & c, const int level_lo )
{
  c.best_level = level_lo; c.evaluated = 0; c.done = 0; c.pad = 0; c.best_score = -1.0;
}

// One round: scores[i] is level first_level + i's, n of them; level_hi is the search's last level.  Scores behind the one that ends the
// search are not looked at.
AA_LFC_HD void lf_choice_round( LfChoice & c, const int first_level, const double * scores, const int n, const int level_hi )
{
  for ( int i = 0; i < n && !c.done; i++ ) {
    c.evaluated++;
    if ( scores[i] > c.best_score ) { c.best_level = first_level + i; c.best_score = scores[i]; }
    else c.done = 1;
  }
  if ( first_level + n > level_hi ) c.done = 1;
}

// Measure 1: the PSNR-like stand-in for SSIM of a plane of pw x ph pixels from its summed squared error, in double precision with
// exactly this grouping.  (Plain divisions and one subtraction: nothing a compiler may contract.)
AA_LFC_HD double lf_sse_score( const uint64_t sse, const uint32_t pw, const uint32_t ph )
{
#if defined( __clang__ )
#pragma clang fp contract( off )
#endif
  const double mean = static_cast<double>( sse ) / ( static_cast<double>( pw ) * ph );
  return 1.0 - mean / ( 255.0 * 255.0 );
}

// What of a stream's segmentation the level of a macroblock depends on
struct LfSegments { int8_t enabled, absolute; int8_t lf[4]; int8_t pad[2]; };

// Four bytes, one per segment: the level a macroblock of that segment is filtered with under header level `level`, zero mode / reference
// adjustments (frame.cc:144-166 and the clamp of macroblock.cc:611-623)
AA_LFC_HD uint32_t lf_segment_levels( const LfSegments & seg, const int level )
{
  uint32_t word = 0;
  for ( int k = 0; k < 4; k++ ) {
    const int v = level ? ( seg.enabled ? seg.lf[k] + ( seg.absolute ? 0 : level ) : level ) : 0;
    word |= static_cast<uint32_t>( v <= 0 ? 0 : ( v > 63 ? 63 : v ) ) << ( 8 * k );
  }
  return word;
}

// An 80-byte macroblock record's first 16 bytes as words x, y (y_mode uv_mode ref_frame segment_id | flags lf_level ...): word y with
// lf_level replaced by the byte of `levels` that belongs to the record's segment
AA_LFC_HD uint32_t lf_relevel_word( const uint32_t x, const uint32_t y, const uint32_t levels )
{
  const uint32_t seg = ( x >> 24 ) & 3u;
  return ( y & 0xFFFF00FFu ) | ( ( ( levels >> ( 8 * seg ) ) & 255u ) << 8 );
}

} // namespace aa
