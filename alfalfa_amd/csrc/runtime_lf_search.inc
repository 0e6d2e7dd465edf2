// runtime.cpp, one of its pieces (ABI): the encoder's loop-filter level search on the GPU (aa_stream_lf_search; its candidates are scored by
// quality_of_planes, runtime_quality.inc), x264's SSIM of planes in host memory (aa_ssim_host) and reference access.
extern "C" {
namespace {
// The reference's choice (encoder.cc:489-503): ascending levels, the first one that does not improve on the best so far ends the search.
void choose_level( const double * q, int n, int level_lo, int * best, double * best_q )
{
  // (the rule itself: lf_choose.hh, shared with k_lf_choose -- all n scores as one round)
  aa::LfChoice c;
  aa::lf_choice_begin( c, level_lo );
  aa::lf_choice_round( c, level_lo, q, n, level_lo + n - 1 );
  *best = c.best_level; *best_q = c.best_score;
}
// what lf_segment_levels (lf_choose.hh) reads of a stream's segmentation
aa::LfSegments lf_segments_of( const aa::SegmentationState & seg, bool enabled )
{
  aa::LfSegments s;
  std::memset( &s, 0, sizeof s );
  s.enabled = enabled; s.absolute = seg.absolute;
  for ( int k = 0; k < 4; k++ ) s.lf[k] = seg.lf[k];
  return s;
}
uint32_t segment_levels( const aa::SegmentationState & seg, int level )      // frame.cc:144-166 + the clamp of macroblock.cc:611-623
{
  return aa::lf_segment_levels( lf_segments_of( seg, seg.enabled ), level );
}

// What a search holds until it returns: its scratch decoders and device memory, which work queued on the compute stream may still use.
struct LfScratch {
  aa_ctx * ctx; std::vector<aa_stream *> streams; uint8_t * dev = nullptr;
  ~LfScratch() { (void) hipStreamSynchronize( ctx->compute ); for ( aa_stream * c : streams ) if ( c ) aa_stream_destroy( c ); if ( dev ) (void) hipFree( dev ); }
};
// A scratch decoder that stands where s stands before this frame: DecoderState and the three references.
aa_status clone_before_frame( aa_stream * s, aa_stream ** out )
{
  if ( aa_status st = aa_stream_create( s->ctx, s->parser.width(), s->parser.height(), out ) ) return st;
  ( *out )->parser = s->parser;
  const void * planes[3][3]; const int is_host[3] = { 0, 0, 0 };
  for ( int r = 0; r < 3; r++ ) for ( int p = 0; p < 3; p++ ) planes[r][p] = slot_plane( s, s->cur_ref_slot[r], p );
  return aa_stream_set_references( *out, planes, is_host );
}
// The end of both routes.  luma: every candidate's padded luma plane, its filtering queued on the compute stream; dev: lf_score_bytes
// of device memory for the original and the n values.  One quality_of_planes call, n doubles come back, then the choice.
size_t lf_score_bytes( const aa_stream * s, int n ) { return align_up( s->plane_bytes[0] ) + size_t( n ) * sizeof( double ); }
aa_status score_and_choose( aa_stream * s, const std::vector<const uint8_t *> & luma, const uint8_t * original_luma, uint8_t * dev,
                            int level_lo, int * best_level, double * best_ssim, double * ssim_out )
{
  aa_ctx * ctx = s->ctx;
  const int n = static_cast<int>( luma.size() );
  double * q_dev = reinterpret_cast<double *>( dev + align_up( s->plane_bytes[0] ) );
  HIP_TRY( hipMemcpyAsync( dev, original_luma, s->plane_bytes[0], hipMemcpyHostToDevice, ctx->compute ) );
  std::vector<QualityPair> pairs( n );
  for ( int i = 0; i < n; i++ ) pairs[i] = { luma[i], s->pw, dev, s->pw, static_cast<uint32_t>( s->pw ), static_cast<uint32_t>( s->ph ) };
  if ( aa_status st = quality_of_planes( ctx, pairs.data(), n, q_dev, nullptr, nullptr ) ) return st;
  std::vector<double> q( n );
  HIP_TRY( hipMemcpyAsync( q.data(), q_dev, q.size() * sizeof( double ), hipMemcpyDeviceToHost, ctx->compute ) );
  HIP_TRY( hipStreamSynchronize( ctx->compute ) );
  if ( aa_status st = check_watchdog( ctx ) ) return st;
  int best; double best_q;
  choose_level( q.data(), n, level_lo, &best, &best_q );
  if ( best_level ) *best_level = best;
  if ( best_ssim ) *best_ssim = best_q;
  if ( ssim_out ) std::copy( q.begin(), q.end(), ssim_out );
  return AA_OK;
}
} // namespace

/* BaseRaster::quality on HOST planes (util/raster.cc:63-66 -> util/ssim.cc:57-71 -> libx264's pixel_ssim_wxh): the same
 * measure k_quality_blocks / k_quality_sum compute on the device (for aa_quality_batch_async and aa_stream_lf_search), for callers
 * that hold rasters in host memory (VP8Raster::quality in the shim).  Plain host arithmetic -- the reference does this on the CPU too. */
aa_status aa_ssim_host( const uint8_t * a, const uint8_t * b, int width, int height, double * out )
{
  if ( !a || !b || !out || width < 8 || height < 8 ) return fail( AA_ERR_ARGUMENT, "aa_ssim_host: null plane or a plane smaller than one 8x8 window" );
  const int w4 = width >> 2, h4 = height >> 2;
  // sums over every 4x4 block: pixels of a, pixels of b, squares of both, products
  std::vector<int> blocks( size_t( w4 ) * h4 * 4 );
  for ( int by = 0; by < h4; by++ )
    for ( int bx = 0; bx < w4; bx++ ) {
      int s1 = 0, s2 = 0, ss = 0, s12 = 0;
      for ( int y = 0; y < 4; y++ ) {
        const uint8_t * pa = a + size_t( 4 * by + y ) * width + 4 * bx, * pb = b + size_t( 4 * by + y ) * width + 4 * bx;
        for ( int x = 0; x < 4; x++ ) { const int p = pa[x], q = pb[x]; s1 += p; s2 += q; ss += p * p + q * q; s12 += p * q; }
      }
      int * t = &blocks[( size_t( by ) * w4 + bx ) * 4];
      t[0] = s1; t[1] = s2; t[2] = ss; t[3] = s12;
    }
  // one term per 8x8 window (2x2 blocks, windows step by 4 pixels), in single precision as x264's ssim_end1
  std::vector<float> win( size_t( w4 - 1 ) * ( h4 - 1 ) );
  for ( int y = 0; y < h4 - 1; y++ )
    for ( int x = 0; x < w4 - 1; x++ ) {
      int v[4];
      for ( int k = 0; k < 4; k++ )
        v[k] = blocks[( size_t( y ) * w4 + x ) * 4 + k] + blocks[( size_t( y ) * w4 + x + 1 ) * 4 + k]
               + blocks[( size_t( y + 1 ) * w4 + x ) * 4 + k] + blocks[( size_t( y + 1 ) * w4 + x + 1 ) * 4 + k];
      const int c1 = 416, c2 = 235963;           // (int)(.01*.01*255*255*64 + .5), (int)(.03*.03*255*255*64*63 + .5)
      const int vars = v[2] * 64 - v[0] * v[0] - v[1] * v[1], covar = v[3] * 64 - v[0] * v[1];
      const float num = static_cast<float>( 2 * v[0] * v[1] + c1 ) * static_cast<float>( 2 * covar + c2 );
      const float den = static_cast<float>( v[0] * v[0] + v[1] * v[1] + c1 ) * static_cast<float>( vars + c2 );
      win[size_t( y ) * ( w4 - 1 ) + x] = num / den;
    }
  // x264's pixel_ssim_wxh: four neighbouring terms left to right into a float, those parts one after another, row after row, into
  // one float total; the mean in double precision.  The order is part of the value.
  float total = 0.0f;
  for ( int y = 0; y < h4 - 1; y++ )
    for ( int x = 0; x < w4 - 1; x += 4 ) {
      float part = 0.0f;
      for ( int k = x; k < std::min( x + 4, w4 - 1 ); k++ ) part += win[size_t( y ) * ( w4 - 1 ) + k];
      total += part;
    }
  *out = static_cast<double>( total ) / static_cast<double>( win.size() );
  return AA_OK;
}

// The search under the diagonal schedule (no row-pipelined filter): every candidate is decoded by a scratch decoder of its own.
static aa_status lf_search_by_decoders( aa_stream * s, const uint8_t * data, size_t size, const uint8_t * original_luma,
                                        int level_lo, int level_hi, int * best_level, double * best_ssim, double * ssim_out, uint8_t * rasters_out )
{
  aa_ctx * ctx = s->ctx;
  const int n = level_hi - level_lo + 1;
  LfScratch scratch { ctx, std::vector<aa_stream *>( n, nullptr ) };
  std::vector<aa_stream *> & cand = scratch.streams;
  std::vector<int> fis( n, -1 );
  const size_t job_bytes = align_up( sizeof( aa_dev_frame ) );
  for ( int i = 0; i < n; i++ ) {
    const int level = level_lo + i;
    if ( aa_status st = clone_before_frame( s, &cand[i] ) ) return st;
    aa_stream * c = cand[i];
    if ( aa_status st = aa_stream_parse( c, data, size, &fis[i], nullptr ) ) return st;
    FrameRec & r = c->frames[fis[i]];
    // the candidate's header: this level, adjustments present and zero.  Per macroblock: the segment's level (frame.cc:144-166)
    // clamped to 0..63 (macroblock.cc:611-623), nothing added (loopfilter.cc:59-79 with zero adjustments).
    const uint32_t seg_level = segment_levels( c->parser.segmentation(), level );
    aa_mb_info * mbs = reinterpret_cast<aa_mb_info *>( reinterpret_cast<uint8_t *>( r.host_job ) + job_bytes );
    for ( unsigned m = 0; m < r.hdr.num_macroblocks; m++ ) mbs[m].lf_level = static_cast<uint8_t>( ( seg_level >> ( 8 * ( mbs[m].segment_id & 3 ) ) ) & 255u );
    r.hdr.loop_filter_level = static_cast<uint8_t>( level );
    r.host_job->loop_filter_level = static_cast<uint8_t>( level );
  }
  if ( aa_status st = aa_decode_batch( ctx, cand.data(), n, fis.data() ) ) return st;
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( &scratch.dev ), lf_score_bytes( s, n ) ) );
  std::vector<const uint8_t *> luma( n );
  for ( int i = 0; i < n; i++ ) luma[i] = slot_plane( cand[i], cand[i]->frames[fis[i]].out_slot, 0 );
  if ( aa_status st = score_and_choose( s, luma, original_luma, scratch.dev, level_lo, best_level, best_ssim, ssim_out ) ) return st;
  if ( rasters_out )
    for ( int i = 0; i < n; i++ ) {
      uint8_t * dst = rasters_out + size_t( i ) * ( s->plane_bytes[0] + 2 * s->plane_bytes[1] );
      if ( aa_status st = aa_stream_download( cand[i], fis[i], dst, dst + s->plane_bytes[0], dst + s->plane_bytes[0] + s->plane_bytes[1] ) ) return st;
    }
  return AA_OK;
}

/* Encoder feedback (SURVEY 8f.4), the loop-filter level search of Encoder::apply_best_loopfilter_settings
 * (encoder.cc:459-516): the frame as serialised with ANY level is parsed and reconstructed ONCE, unfiltered, on a scratch copy
 * of the decoder (state + references; the stream itself is untouched).  Every candidate level then is an independent frame
 * for the loop filter: a copy of the unfiltered raster, the macroblock records with the candidate's per-segment level and zero
 * mode / reference adjustments (`filter_adjustments.reset( frame.header() )` after the adjustments were zeroed,
 * encoder.cc:464-470) -- ONE k_loopfilter_rows4 launch over all candidates -- scored with BaseRaster::quality = x264's SSIM of
 * the padded luma planes (util/raster.cc:63-66, util/ssim.cc:57-71): all candidates in ONE quality_of_planes call, one double
 * each comes back.  Selection as in the reference: levels in ascending order, the first one that does not improve on the best so
 * far ends the search (encoder.cc:489-503).
 * (With the diagonal schedule -- no row-pipelined filter -- every candidate is decoded by a scratch decoder of its own.) */
aa_status aa_stream_lf_search( aa_stream * s, const uint8_t * data, size_t size, const uint8_t * original_luma,
                               int level_lo, int level_hi, int * best_level, double * best_ssim, double * ssim_out, uint8_t * rasters_out )
{
  if ( !s || !data || !original_luma ) return fail( AA_ERR_ARGUMENT, "aa_stream_lf_search: null argument" );
  if ( level_lo < 0 || level_hi > 63 || level_lo > level_hi ) return fail( AA_ERR_ARGUMENT, "aa_stream_lf_search: levels must be 0 <= lo <= hi <= 63" );
  aa_ctx * ctx = s->ctx;
  if ( aa_status st = set_device( ctx ) ) return st;
  if ( s->next_submit != static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_LOGIC, "aa_stream_lf_search: parsed frames are still waiting to be decoded" );
  if ( aa_status st = segmap_to_host( s ) ) return st;
  if ( ctx->schedule != 0 ) return lf_search_by_decoders( s, data, size, original_luma, level_lo, level_hi, best_level, best_ssim, ssim_out, rasters_out );
  const int n = level_hi - level_lo + 1;

  // ---- the unfiltered reconstruction, on a scratch decoder ----
  LfScratch scratch { ctx, std::vector<aa_stream *>( 1, nullptr ) };
  if ( aa_status st = clone_before_frame( s, &scratch.streams[0] ) ) return st;
  aa_stream * x = scratch.streams[0];
  int fx = -1;
  if ( aa_status st = aa_stream_parse( x, data, size, &fx, nullptr ) ) return st;
  {
    FrameRec & r = x->frames[fx];
    r.hdr.loop_filter_level = 0; r.host_job->loop_filter_level = 0;      // Frame::decode only (frame.cc:208-250)
  }
  if ( aa_status st = aa_decode_batch( ctx, &x, 1, &fx ) ) return st;
  const FrameRec & rx = x->frames[fx];
  const aa_dev_frame job_x = *rx.host_job;
  const unsigned nmb = rx.hdr.num_macroblocks;
  const uint8_t * unfiltered = slot_plane( x, rx.out_slot, 0 );
  const size_t raster_bytes = s->plane_bytes[0] + 2 * s->plane_bytes[1];

  // ---- per candidate: raster | macroblock records | job; then the original and the scores ----
  const size_t mb_bytes = align_up( size_t( nmb ) * sizeof( aa_mb_info ) ), job_bytes = align_up( sizeof( aa_dev_frame ) );
  const size_t per = align_up( raster_bytes ) + mb_bytes + job_bytes;
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( &scratch.dev ), per * n + lf_score_bytes( s, n ) ) );
  uint8_t * base = scratch.dev;
  std::vector<aa_dev_frame> jobs( n );
  std::vector<std::pair<uint32_t, const aa_dev_frame *>> keyed;
  std::vector<const uint8_t *> luma( n );
  for ( int i = 0; i < n; i++ ) {
    const int level = level_lo + i;
    uint8_t * raster = base + per * i;
    aa_mb_info * mbs = reinterpret_cast<aa_mb_info *>( raster + align_up( raster_bytes ) );
    aa_dev_frame * job_dev = reinterpret_cast<aa_dev_frame *>( reinterpret_cast<uint8_t *>( mbs ) + mb_bytes );
    luma[i] = level ? raster : unfiltered;                               // level 0: Frame::loopfilter does nothing (frame.cc:144)
    if ( !level ) continue;
    HIP_TRY( hipMemcpyAsync( raster, unfiltered, raster_bytes, hipMemcpyDeviceToDevice, ctx->compute ) );
    if ( const int e = aa::launch_lf_relevel( job_x.mbs, mbs, nmb, segment_levels( x->parser.segmentation(), level ), ctx->compute ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_lf_relevel" );
    jobs[i] = job_x;
    jobs[i].cur[0] = raster; jobs[i].cur[1] = raster + s->plane_bytes[0]; jobs[i].cur[2] = raster + s->plane_bytes[0] + s->plane_bytes[1];
    jobs[i].mbs = mbs;
    jobs[i].loop_filter_level = static_cast<uint8_t>( level );
    HIP_TRY( hipMemcpyAsync( job_dev, &jobs[i], sizeof( aa_dev_frame ), hipMemcpyHostToDevice, ctx->compute ) );
    keyed.emplace_back( ( static_cast<uint32_t>( rx.hdr.mb_width ) << 16 ) | rx.hdr.mb_height, job_dev );
  }
  if ( !keyed.empty() ) if ( aa_status st = launch_lf_rows( ctx, keyed, true, rx.hdr.mb_height, rx.hdr.mb_width ) ) return st;
  if ( aa_status st = score_and_choose( s, luma, original_luma, base + per * n, level_lo, best_level, best_ssim, ssim_out ) ) return st;
  if ( rasters_out )
    for ( int i = 0; i < n; i++ ) HIP_TRY( hipMemcpy( rasters_out + raster_bytes * i, luma[i], raster_bytes, hipMemcpyDeviceToHost ) );
  return AA_OK;
}

/* Device planes of References::last / golden / alternative as they stand (which: 0, 1, 2) */
aa_status aa_stream_reference_device( aa_stream * s, int which, void ** y, void ** u, void ** v )
{
  if ( !s || which < 0 || which > 2 ) return fail( AA_ERR_ARGUMENT, "aa_stream_reference_device: bad argument" );
  const int slot = s->cur_ref_slot[which];
  if ( y ) *y = slot_plane( s, slot, 0 );
  if ( u ) *u = slot_plane( s, slot, 1 );
  if ( v ) *v = slot_plane( s, slot, 2 );
  return AA_OK;
}
aa_status aa_stream_reference_download( aa_stream * s, int which, uint8_t * y, uint8_t * u, uint8_t * v )
{
  if ( !s || which < 0 || which > 2 ) return fail( AA_ERR_ARGUMENT, "aa_stream_reference_download: bad argument" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  HIP_TRY( hipStreamSynchronize( s->ctx->compute ) );
  if ( aa_status st = check_watchdog( s->ctx ) ) return st;
  uint8_t * dst[3] = { y, u, v };
  for ( int p = 0; p < 3; p++ ) if ( dst[p] ) HIP_TRY( hipMemcpy( dst[p], slot_plane( s, s->cur_ref_slot[which], p ), s->plane_bytes[p], hipMemcpyDeviceToHost ) );
  return AA_OK;
}

} // extern "C"
