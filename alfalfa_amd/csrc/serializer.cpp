// Host half of the serialisation (see serializer.hh for the reference functions it restates).
#include "serializer.hh"

#include <cstring>
#include <memory>
#include <string>

#include "bool_writer.hh"
#include "serialize_common.hh"

namespace aa {

namespace {

// Tree<>::encode (encode_tree.cc): the branches from the root to the leaf that holds `value`, each with its node's probability.
// Trees as parse_common.hh stores them: leaves as -value, inner nodes as positive even indices.
bool tree_path( const int8_t * nodes, int at, int value, uint8_t * node_of, uint8_t * bit_of, int & depth )
{
  for ( int b = 0; b < 2; b++ ) {
    const int t = nodes[at + b];
    node_of[depth] = static_cast<uint8_t>( at ); bit_of[depth] = static_cast<uint8_t>( b ); depth++;
    if ( t <= 0 ? -t == value : tree_path( nodes, t, value, node_of, bit_of, depth ) ) return true;
    depth--;
  }
  return false;
}
void put_tree( BoolWriter & w, const int8_t * nodes, const uint8_t * probs, int value )
{
  uint8_t node_of[16], bit_of[16];
  int depth = 0;
  if ( !tree_path( nodes, 0, value, node_of, bit_of, depth ) ) throw ParseError( AA_ERR_ARGUMENT, "serialize: a macroblock record holds a value its tree has no leaf for" );
  for ( int i = 0; i < depth; i++ ) w.put( bit_of[i], probs[node_of[i] >> 1] );
}

void put_flagged_signed( BoolWriter & w, int present, int value, int bits )
{
  w.put( present != 0 );
  if ( present ) w.signed_literal( value, bits );
}

// encode( KeyFrameHeader ) / encode( InterFrameHeader ), serializer.cc:140-181
void write_frame_header( BoolWriter & w, const aa_frame_header & h, const aa_frame_header_ext & x )
{
  const bool key = h.key_frame;
  if ( key ) { w.put( x.color_space ); w.put( x.clamping_type ); }
  w.put( h.segmentation_enabled );                               // Flagged<UpdateSegmentation>
  if ( h.segmentation_enabled ) {
    w.put( x.update_mb_segmentation_map );
    w.put( x.update_segment_feature_data );
    if ( x.update_segment_feature_data ) {
      w.put( x.segment_feature_mode );
      for ( int i = 0; i < 4; i++ ) put_flagged_signed( w, x.seg_quant_update[i], x.seg_quant[i], 7 );
      for ( int i = 0; i < 4; i++ ) put_flagged_signed( w, x.seg_lf_update[i], x.seg_lf[i], 6 );
    }
    if ( x.update_mb_segmentation_map )
      for ( int i = 0; i < 3; i++ ) { w.put( x.seg_tree_update[i] != 0 ); if ( x.seg_tree_update[i] ) w.literal( x.seg_tree_probs[i], 8 ); }
  }
  w.put( x.filter_type );
  w.literal( h.loop_filter_level, 6 );
  w.literal( h.sharpness_level, 3 );
  w.put( h.filter_adjustments_enabled );                         // Flagged<Flagged<ModeRefLFDeltaUpdate>>
  if ( h.filter_adjustments_enabled ) {
    w.put( x.lf_delta_update );
    if ( x.lf_delta_update ) {
      for ( int i = 0; i < 4; i++ ) put_flagged_signed( w, x.ref_lf_update[i], x.ref_lf_delta[i], 6 );
      for ( int i = 0; i < 4; i++ ) put_flagged_signed( w, x.mode_lf_update[i], x.mode_lf_delta[i], 6 );
    }
  }
  const int log2_parts = h.num_dct_partitions == 8 ? 3 : ( h.num_dct_partitions == 4 ? 2 : ( h.num_dct_partitions == 2 ? 1 : 0 ) );
  w.literal( static_cast<uint32_t>( log2_parts ), 2 );
  w.literal( h.q_index, 7 );
  for ( int i = 0; i < 5; i++ ) put_flagged_signed( w, x.q_update[i], x.q_delta[i], 4 );
  if ( key ) w.put( x.refresh_entropy_probs );
  else {
    w.put( h.refresh_golden ); w.put( h.refresh_alternate );
    if ( !h.refresh_golden ) w.literal( h.copy_buffer_to_golden, 2 );
    if ( !h.refresh_alternate ) w.literal( h.copy_buffer_to_alternate, 2 );
    w.put( h.sign_bias_golden ); w.put( h.sign_bias_alternate );
    w.put( x.refresh_entropy_probs );
    w.put( h.refresh_last );
  }
  const uint8_t * up = &x.token_prob_update[0][0][0][0], * val = &x.token_prob[0][0][0][0];
  for ( int i = 0; i < 1056; i++ ) {
    w.put( up[i] != 0, k_coeff_update_probs[i] );
    if ( up[i] ) w.literal( val[i], 8 );
  }
  w.put( x.skip_enabled );
  if ( x.skip_enabled ) w.literal( x.prob_skip_false, 8 );
  if ( !key ) {
    w.literal( x.prob_inter, 8 ); w.literal( x.prob_references_last, 8 ); w.literal( x.prob_references_golden, 8 );
    w.put( x.intra_16x16_update );
    if ( x.intra_16x16_update ) for ( int i = 0; i < 4; i++ ) w.literal( x.intra_16x16_prob[i], 8 );
    w.put( x.intra_chroma_update );
    if ( x.intra_chroma_update ) for ( int i = 0; i < 3; i++ ) w.literal( x.intra_chroma_prob[i], 8 );
    for ( int i = 0; i < 2; i++ ) for ( int j = 0; j < 19; j++ ) {
      w.put( x.mv_prob_update[i][j] != 0, k_mv_update_probs[i * 19 + j] );
      if ( x.mv_prob_update[i][j] ) w.literal( x.mv_prob[i][j], 7 );
    }
  }
}

// encode( int16_t, component_probs ), serializer.cc:196-237 (the writing half of read_mv_component)
void put_mv_component( BoolWriter & w, int num, const uint8_t * p )
{
  enum { MV_IS_SHORT, SIGN, SHORT, BITS = SHORT + 8 - 1, MV_LONG_BITS = 10 };
  const int n = num >> 1;
  const unsigned x = static_cast<unsigned>( n < 0 ? -n : n ) & 0xFFFFu;
  if ( x < 8 ) {
    w.put( 0, p[MV_IS_SHORT] );
    put_tree( w, kSmallMvTree, p + SHORT, static_cast<int>( x ) );
  } else {
    w.put( 1, p[MV_IS_SHORT] );
    for ( int i = 0; i < 3; i++ ) w.put( ( x >> i ) & 1u, p[BITS + i] );
    for ( int i = MV_LONG_BITS - 1; i > 3; i-- ) w.put( ( x >> i ) & 1u, p[BITS + i] );
    if ( x & 0xFFF0u ) w.put( ( x >> 3 ) & 1u, p[BITS + 3] );
  }
  if ( x ) w.put( n < 0, p[SIGN] );
}
void put_mv( BoolWriter & w, const Mv & m, const ProbTables & t )
{
  put_mv_component( w, m.y, t.mv[0] );   // row first (serializer.cc:239-245)
  put_mv_component( w, m.x, t.mv[1] );
}

Mv mv_of( const aa_mb_info & mb, int b ) { Mv m; m.x = mb.u.mv[b][0]; m.y = mb.u.mv[b][1]; return m; }

// Macroblock::serialize (serializer.cc:370-385) + encode_prediction_modes (:285-368) for macroblock (col, row)
void write_mb_header( BoolWriter & w, const aa_frame_header & h, const aa_frame_header_ext & x, const HeaderParams & fp, const ProbTables & t,
                      const aa_mb_info * mbs, unsigned col, unsigned row, const uint8_t * sub_modes, size_t n_sub_modes, size_t & sub_at )
{
  const HeaderTables & T = kHeaderTables;
  const unsigned mbw = h.mb_width, mbh = h.mb_height, mi = row * mbw + col;
  const aa_mb_info & mb = mbs[mi];
  const bool key = h.key_frame, inter = mb.flags & AA_MB_INTER;
  if ( mb.y_mode > SPLITMV || mb.uv_mode > TM_PRED || mb.ref_frame > ALTREF_FRAME || mb.segment_id > 3 || ( inter && key )
       || inter != ( mb.ref_frame != CURRENT_FRAME ) || inter != ( mb.y_mode > B_PRED ) )
    throw ParseError( AA_ERR_ARGUMENT, "serialize: macroblock " + std::to_string( mi ) + " has fields no frame of this kind can say" );
  if ( h.segmentation_enabled && x.update_mb_segmentation_map ) put_tree( w, T.segment_id_tree, x.seg_tree_probs, mb.segment_id );
  if ( x.skip_enabled ) w.put( ( mb.flags & AA_MB_SKIP ) != 0, x.prob_skip_false );
  if ( !key ) {
    w.put( inter, x.prob_inter );
    if ( inter ) {
      w.put( mb.ref_frame != LAST_FRAME, x.prob_references_last );
      if ( mb.ref_frame != LAST_FRAME ) w.put( mb.ref_frame == ALTREF_FRAME, x.prob_references_golden );
    }
  }
  if ( !inter ) {
    if ( key ) put_tree( w, T.kf_y_mode_tree, T.kf_y_mode_probs, mb.y_mode );
    else put_tree( w, T.y_mode_tree, t.y_mode, mb.y_mode );
    if ( mb.y_mode == B_PRED )
      for ( int b = 0; b < 16; b++ ) {
        if ( mb.u.b_mode[b] > B_HU_PRED ) throw ParseError( AA_ERR_ARGUMENT, "serialize: macroblock " + std::to_string( mi ) + " has a sub-block mode out of range" );
        if ( key ) {
          const int above_mode = b >= 4 ? mb.u.b_mode[b - 4] : ( row > 0 ? mbs[mi - mbw].u.b_mode[12 + b] : B_DC_PRED );
          const int left_mode = ( b & 3 ) ? mb.u.b_mode[b - 1] : ( col > 0 ? mbs[mi - 1].u.b_mode[b + 3] : B_DC_PRED );
          if ( above_mode > B_HU_PRED || left_mode > B_HU_PRED ) throw ParseError( AA_ERR_ARGUMENT, "serialize: macroblock " + std::to_string( mi ) + " has a neighbour's sub-block mode out of range" );
          put_tree( w, T.b_mode_tree, T.kf_b_mode_probs + ( above_mode * 10 + left_mode ) * 9, mb.u.b_mode[b] );
        } else put_tree( w, T.b_mode_tree, T.b_mode_probs, mb.u.b_mode[b] );
      }
    if ( key ) put_tree( w, T.uv_mode_tree, T.kf_uv_mode_probs, mb.uv_mode );
    else put_tree( w, T.uv_mode_tree, t.uv_mode, mb.uv_mode );
    return;
  }
  // ---- the census, as parse_mb_header takes it (scorer.hh, macroblock.cc:143-181,301-312) ----
  uint8_t score[4] = { 0, 0, 0, 0 };
  Mv cand[4];
  int idx = 0, split_score = 0;
  const bool my_flip = mv_flipped( fp, mb.ref_frame );
  auto consider = [&]( unsigned ni, int weight ) {
    const aa_mb_info & nb = mbs[ni];
    if ( !( nb.flags & AA_MB_INTER ) ) return;
    Mv mv = mv_of( nb, 15 );
    if ( mv_flipped( fp, nb.ref_frame ) != my_flip ) { mv.x = static_cast<int16_t>( -mv.x ); mv.y = static_cast<int16_t>( -mv.y ); }
    if ( mv.zero() ) score[0] += weight;
    else {
      if ( !( mv == cand[idx] ) ) cand[++idx] = mv;
      score[idx] += weight;
    }
    if ( nb.y_mode == SPLITMV ) split_score += weight;
  };
  if ( row > 0 ) consider( mi - mbw, 2 );
  if ( col > 0 ) consider( mi - 1, 2 );
  if ( row > 0 && col > 0 ) consider( mi - mbw - 1, 1 );
  if ( score[3] && cand[idx] == cand[1] ) score[1] += score[3];
  if ( score[2] > score[1] ) {
    const uint8_t ts = score[1]; score[1] = score[2]; score[2] = ts;
    const Mv tm = cand[1]; cand[1] = cand[2]; cand[2] = tm;
  }
  if ( score[1] >= score[0] ) cand[0] = cand[1];
  const uint8_t mode_probs[4] = { T.mv_counts_to_probs[score[0] * 4 + 0], T.mv_counts_to_probs[score[1] * 4 + 1],
                                  T.mv_counts_to_probs[score[2] * 4 + 2], T.mv_counts_to_probs[split_score * 4 + 3] };
  put_tree( w, T.mv_ref_tree, mode_probs, mb.y_mode );
  const Mv best = clamp_mv( cand[0], col, row, mbw, mbh );
  if ( mb.y_mode == NEWMV ) {
    Mv d = mv_of( mb, 0 );
    d.x = static_cast<int16_t>( d.x - best.x ); d.y = static_cast<int16_t>( d.y - best.y );
    put_mv( w, d, t );
  } else if ( mb.y_mode == SPLITMV ) {
    if ( mb.split_partition > 3 ) throw ParseError( AA_ERR_ARGUMENT, "serialize: macroblock " + std::to_string( mi ) + " has a split partition out of range" );
    put_tree( w, T.split_mv_tree, T.split_mv_probs, mb.split_partition );
    for ( int part = 0; part < T.split_count[mb.split_partition]; part++ ) {
      const int b = T.split_first[mb.split_partition][part];
      // YBlock::write_subblock_inter_prediction (serializer.cc:247-283).  The records hold the vector, not the sub-block mode that said
      // it: the caller's list says it where it can (serializer.hh), else the first of LEFT4X4, ABOVE4X4, ZERO4X4 that gives the vector
      // is written, NEW4X4 otherwise.
      Mv lmv, amv;
      if ( b & 3 ) lmv = mv_of( mb, b - 1 );
      else if ( col > 0 && ( mbs[mi - 1].flags & AA_MB_INTER ) ) lmv = mv_of( mbs[mi - 1], b + 3 );
      if ( b >= 4 ) amv = mv_of( mb, b - 4 );
      else if ( row > 0 && ( mbs[mi - mbw].flags & AA_MB_INTER ) ) amv = mv_of( mbs[mi - mbw], b + 12 );
      int ctx = 0;
      if ( lmv == amv ) ctx = lmv.zero() ? 4 : 3;
      else if ( amv.zero() ) ctx = 2;
      else if ( lmv.zero() ) ctx = 1;
      const Mv m = mv_of( mb, b );
      int sub = m == lmv ? LEFT4X4 : ( m == amv ? ABOVE4X4 : ( m.zero() ? ZERO4X4 : NEW4X4 ) );
      if ( sub_modes && sub_at < n_sub_modes ) {
        const int said = sub_modes[sub_at++];
        if ( said == NEW4X4 || ( said == LEFT4X4 && m == lmv ) || ( said == ABOVE4X4 && m == amv ) || ( said == ZERO4X4 && m.zero() ) ) sub = said;
      }
      put_tree( w, T.sub_mv_ref_tree, T.submv_ref_probs + ctx * 3, sub );
      if ( sub == NEW4X4 ) {
        Mv d = m;
        d.x = static_cast<int16_t>( d.x - best.x ); d.y = static_cast<int16_t>( d.y - best.y );
        put_mv( w, d, t );
      }
    }
  }
}

} // namespace

void frame_probs( const uint8_t * before, bool key_frame, const aa_frame_header_ext & x, ProbTables & out )
{
  if ( key_frame ) out.set_defaults();
  else {
    std::memcpy( out.coeff, before, 1056 ); std::memcpy( out.y_mode, before + 1056, 4 );
    std::memcpy( out.uv_mode, before + 1060, 3 ); std::memcpy( out.mv, before + 1063, 38 );
  }
  uint8_t * c = &out.coeff[0][0][0][0];
  const uint8_t * up = &x.token_prob_update[0][0][0][0], * val = &x.token_prob[0][0][0][0];
  for ( int i = 0; i < 1056; i++ ) if ( up[i] ) c[i] = val[i];
  if ( key_frame ) return;
  if ( x.intra_16x16_update ) std::memcpy( out.y_mode, x.intra_16x16_prob, 4 );
  if ( x.intra_chroma_update ) std::memcpy( out.uv_mode, x.intra_chroma_prob, 3 );
  for ( int i = 0; i < 2; i++ ) for ( int j = 0; j < 19; j++ )
    if ( x.mv_prob_update[i][j] ) out.mv[i][j] = static_cast<uint8_t>( x.mv_prob[i][j] ? x.mv_prob[i][j] << 1 : 1 );
}

void write_first_partition( const aa_frame_header & h, const aa_frame_header_ext & x, const ProbTables & t, const aa_mb_info * mbs, const uint8_t * sub_modes, size_t n_sub_modes,
                            std::vector<uint8_t> & out )
{
  // room: the frame header is at most ~1.4 KB (1056 flagged bytes); a macroblock header at most 16 sub-block vectors of two long components
  // (16 x 2 x 12 bools) plus modes, well under 1 KB at 7 bits a bool
  const size_t nmb = static_cast<size_t>( h.mb_width ) * h.mb_height;
  out.assign( 4096 + nmb * 1024, 0 );
  BoolWriter w( out.data(), static_cast<uint32_t>( out.size() ) );
  write_frame_header( w, h, x );
  HeaderParams fp {};
  fp.sign_bias_golden = h.sign_bias_golden; fp.sign_bias_alt = h.sign_bias_alternate;
  size_t sub_at = 0;
  for ( unsigned row = 0; row < h.mb_height; row++ )
    for ( unsigned col = 0; col < h.mb_width; col++ ) write_mb_header( w, h, x, fp, t, mbs, col, row, sub_modes, n_sub_modes, sub_at );
  const uint32_t size = w.finish();
  if ( !w.fits() ) throw ParseError( AA_ERR_LOGIC, "serialize: the first partition outgrew its worst case" );
  out.resize( size );
}

size_t assemble_frame( const aa_frame_header & h, const std::vector<uint8_t> & first, const uint8_t * const * parts, const uint32_t * sizes, uint8_t * out, size_t capacity )
{
  const unsigned nparts = h.num_dct_partitions;
  size_t total = ( h.key_frame ? 10u : 3u ) + first.size() + 3u * ( nparts - 1 );
  for ( unsigned i = 0; i < nparts; i++ ) total += sizes[i];
  if ( total > capacity ) return total;
  const uint32_t len = static_cast<uint32_t>( first.size() );
  uint8_t * p = out;
  *p++ = static_cast<uint8_t>( ( h.key_frame ? 0 : 1 ) | ( ( h.show_frame ? 1 : 0 ) << 4 ) | ( ( len & 7u ) << 5 ) );
  *p++ = static_cast<uint8_t>( ( len & 0x7F8u ) >> 3 );
  *p++ = static_cast<uint8_t>( ( len & 0x7F800u ) >> 11 );
  if ( h.key_frame ) {
    *p++ = 0x9d; *p++ = 0x01; *p++ = 0x2a;
    *p++ = static_cast<uint8_t>( h.width & 0xFF ); *p++ = static_cast<uint8_t>( ( h.width & 0x3F00 ) >> 8 );
    *p++ = static_cast<uint8_t>( h.height & 0xFF ); *p++ = static_cast<uint8_t>( ( h.height & 0x3F00 ) >> 8 );
  }
  if ( len ) std::memcpy( p, first.data(), len );
  p += len;
  for ( unsigned i = 0; i + 1 < nparts; i++ ) { *p++ = static_cast<uint8_t>( sizes[i] ); *p++ = static_cast<uint8_t>( sizes[i] >> 8 ); *p++ = static_cast<uint8_t>( sizes[i] >> 16 ); }
  for ( unsigned i = 0; i < nparts; i++ ) { if ( sizes[i] ) std::memcpy( p, parts[i], sizes[i] ); p += sizes[i]; }
  return total;
}

size_t estimate_frame_bytes( bool key_frame, uint16_t small_w, uint16_t small_h, uint8_t q_index, const uint8_t * probs_before, const aa_mb_info * recs, const uint32_t * masks,
                             uint32_t token_bytes, uint32_t with_coefficients, uint32_t intra, uint8_t carry[4] )
{
  aa_frame_header h;
  std::memset( &h, 0, sizeof h );
  h.key_frame = key_frame; h.show_frame = 1; h.num_dct_partitions = 1; h.q_index = q_index;
  h.refresh_last = 1; h.refresh_golden = h.refresh_alternate = key_frame;
  h.width = small_w; h.height = small_h;
  h.mb_width = static_cast<uint16_t>( ( small_w + 15 ) / 16 ); h.mb_height = static_cast<uint16_t>( ( small_h + 15 ) / 16 );
  const uint32_t nmb = static_cast<uint32_t>( h.mb_width ) * h.mb_height;
  h.num_macroblocks = nmb;
  std::unique_ptr<aa_frame_header_ext> xp( new aa_frame_header_ext );
  aa_frame_header_ext & x = *xp;
  std::memset( &x, 0, sizeof x );
  x.refresh_entropy_probs = 1;
  x.skip_enabled = 1; x.prob_skip_false = static_cast<uint8_t>( ser::calc_prob( with_coefficients, nmb ) );          // optimize_prob_skip
  if ( !key_frame ) {
    // optimize_interframe_probs (encode_inter.cc:525-575): every inter macroblock is on LAST, so prob_references_golden's count is 0 / 0
    const uint32_t prob_inter = ser::calc_prob( intra, nmb ), prob_last = ser::calc_prob( nmb - intra, nmb - intra );
    if ( prob_inter > 0 ) carry[0] = static_cast<uint8_t>( prob_inter );
    if ( prob_last > 0 ) carry[1] = static_cast<uint8_t>( prob_last );
    x.prob_inter = carry[0]; x.prob_references_last = carry[1]; x.prob_references_golden = carry[2];
  }
  // the records as the first partition reads them: modes, vectors, the inter and the skip flag
  std::vector<aa_mb_info> mbs( recs, recs + nmb );
  for ( uint32_t i = 0; i < nmb; i++ ) {
    aa_mb_info & m = mbs[i];
    const bool inter = m.ref_frame != 0, y2 = m.y_mode != B_PRED && m.y_mode != SPLITMV;
    const uint32_t mask = masks[i] & ( y2 ? 0x1FFFFFFu : 0xFFFFFFu );
    m.flags = static_cast<uint8_t>( ( inter ? AA_MB_INTER : 0u ) | ( y2 ? AA_MB_HAS_Y2 : 0u ) | ( mask ? AA_MB_HAS_NONZERO : AA_MB_SKIP ) );
    m.nz_mask = mask; m.segment_id = 0;
  }
  ProbTables t;
  frame_probs( probs_before, key_frame, x, t );
  std::vector<uint8_t> first;
  write_first_partition( h, x, t, mbs.data(), nullptr, 0, first );
  return ( key_frame ? 10u : 3u ) + first.size() + token_bytes;
}

void serialize_frame_host( const aa_frame_header & h, const aa_frame_header_ext & x, const uint8_t * probs_before, const aa_mb_info * mbs, const int16_t * coeffs,
                           const uint8_t * sub_modes, size_t n_sub_modes, std::vector<uint8_t> & out )
{
  const unsigned nparts = h.num_dct_partitions;
  if ( nparts != 1 && nparts != 2 && nparts != 4 && nparts != 8 ) throw ParseError( AA_ERR_ARGUMENT, "serialize: num_dct_partitions must be 1, 2, 4 or 8" );
  ProbTables t;
  frame_probs( probs_before, h.key_frame, x, t );
  std::vector<uint8_t> first;
  write_first_partition( h, x, t, mbs, sub_modes, n_sub_modes, first );
  // a partition's worst case: 25 blocks x 16 tokens x 20 bools x 7 bits per macroblock of its rows, and the flush
  std::unique_ptr<uint8_t[]> parts[8];          // (not zero-filled: a partition touches what it writes, not its worst case)
  const uint8_t * ptr[8]; uint32_t sizes[8];
  for ( unsigned p = 0; p < nparts; p++ ) {
    const size_t rows = ( h.mb_height + nparts - 1 - p ) / nparts;
    const size_t room = 16 + rows * h.mb_width * 7000;
    parts[p].reset( new uint8_t[room] );
    BoolWriter w( parts[p].get(), static_cast<uint32_t>( room ) );
    sizes[p] = ser::write_partition( w, &t.coeff[0][0][0][0], mbs, h.mb_width, h.mb_height, coeffs, false, x.skip_enabled != 0, p, nparts );
    if ( !w.fits() ) throw ParseError( AA_ERR_LOGIC, "serialize: a DCT partition outgrew its worst case" );
    ptr[p] = parts[p].get();
  }
  const size_t total = assemble_frame( h, first, ptr, sizes, nullptr, 0 );
  out.assign( total, 0 );
  assemble_frame( h, first, ptr, sizes, out.data(), total );
}

} // namespace aa
