// The compaction rule of a rebased frame's records, one source for host and device: what rebase_records (runtime_rebase.inc) does per
// macroblock with the masks and dense slots the rebase kernels leave, stated as pure functions so that k_rebase_count / k_rebase_compact
// (rebase_compact_kernels.hip) and tests/cpp/rebase_compact_check.cc compile the same text.
//
// A macroblock's stored blocks follow each other in PARSE order -- the Y2 block (slot 24) first if it is stored, then slots 0..23
// ascending -- and a frame's macroblocks follow each other in raster order: coeff_index is the exclusive prefix sum of the stored masks'
// populations.  The kernels take that sum in runs of kCompactMbs macroblocks, a workgroup each: k_rebase_count leaves one word per run,
// a run's first index is the sum of the words before it (run_base), and a scan inside the run gives the rest.
#pragma once
#include <stdint.h>

#include "../../include/alfalfa_amd.h"
#include "vp8_math.hh"      // AA_MHD

namespace aa {
namespace compact {

constexpr uint32_t kCompactMbs = 256;          // macroblocks per workgroup of the two kernels, one thread each
constexpr uint32_t kSlots = 25;                // dense slots per macroblock: 0..15 Y, 16..19 U, 20..23 V, 24 Y2
constexpr uint32_t kUnitsPerMb = kSlots * 2;   // 16-byte halves of a macroblock's slots: what a thread of the copy moves

AA_MHD uint32_t popc( const uint32_t v ) { return static_cast<uint32_t>( __builtin_popcount( v ) ); }
AA_MHD uint32_t runs_of( const uint32_t nmb ) { return ( nmb + kCompactMbs - 1 ) / kCompactMbs; }

// a Y2 block is coded unless the mode is B_PRED (4) or SPLITMV (9)
AA_MHD bool has_y2( const uint32_t y_mode ) { return y_mode != 4 && y_mode != 9; }
// what is stored of the mask the kernels wrote: without a Y2 block bit 24 means nothing
AA_MHD uint32_t stored_mask( const uint32_t raw, const uint32_t y_mode ) { return raw & ( has_y2( y_mode ) ? 0x1FFFFFFu : 0xFFFFFFu ); }
// flags as the parser sets them for the serialised frame: every rebased frame codes mb_skip_coeff = no coefficient left
AA_MHD uint8_t flags_of( const uint32_t ref_frame, const uint32_t y_mode, const uint32_t mask )
{
  const bool y2 = has_y2( y_mode );
  return static_cast<uint8_t>( ( ref_frame != 0 ? AA_MB_INTER : 0u ) | ( y2 ? AA_MB_HAS_Y2 : 0u )
                               | ( mask ? AA_MB_HAS_NONZERO : AA_MB_SKIP | ( y2 ? AA_MB_LF_SKIP_INNER : 0u ) ) );
}
// where the stored slot b of a macroblock lies among that macroblock's blocks
AA_MHD uint32_t place_of( const uint32_t mask, const uint32_t b ) { return b == 24 ? 0u : popc( mask & ( ( 1u << b ) - 1u ) ) + ( mask >> 24 ); }

// the output record: the input's modes, reference, vectors, b_modes, partition, segment and filter level with the residue fields set
AA_MHD aa_mb_info output_record( aa_mb_info m, const uint32_t raw_mask, const uint32_t coeff_index )
{
  const uint32_t mask = stored_mask( raw_mask, m.y_mode );
  m.reserved = 0;
  m.flags = flags_of( m.ref_frame, m.y_mode, mask );
  m.nz_mask = mask;
  m.coeff_index = coeff_index;
  return m;
}

// the first coeff_index of run `run` of a frame: the blocks of the runs before it (partials: k_rebase_count's words of that frame)
AA_MHD uint32_t run_base( const uint32_t * partials, const uint32_t run )
{
  uint32_t base = 0;
  for ( uint32_t r = 0; r < run; r++ ) base += partials[r];
  return base;
}

// Unit u of a run (0 .. macroblocks of the run * kUnitsPerMb): macroblock u / 50 of the run, slot (u % 50) / 2, half (u % 50) % 2.
// -> the unit's byte offset in the dense scratch (from the run's first macroblock) and, if the slot is stored, in the frame's
// coefficient area; false: the slot's mask bit is clear, nothing is loaded or stored.
struct Unit { uint32_t mb, slot, half; };
AA_MHD Unit unit_of( const uint32_t u )
{
  Unit x;
  x.mb = u / kUnitsPerMb;
  const uint32_t r = u - x.mb * kUnitsPerMb;
  x.slot = r >> 1; x.half = r & 1u;
  return x;
}
AA_MHD size_t unit_source( const Unit & x ) { return ( static_cast<size_t>( x.mb ) * kSlots + x.slot ) * 32 + x.half * 16; }
AA_MHD bool unit_stored( const Unit & x, const uint32_t mask ) { return ( mask >> x.slot ) & 1u; }
AA_MHD uint32_t unit_block( const Unit & x, const uint32_t mask, const uint32_t coeff_index ) { return coeff_index + place_of( mask, x.slot ); }

} // namespace compact
} // namespace aa
