// runtime.cpp (ABI): the loop-filter level search of appended frames, batched (aa_lf_search_decode_batch) -- the last statement of
// Encoder::reencode_as_interframe (reencode.cc:126, apply_best_loopfilter_settings, encoder.cc:459-516) for every job at once, and the
// decode of those frames.  aa_stream_lf_search (runtime_lf_search.inc) searches one frame given as BYTES on a scratch decoder, with a copy,
// a k_lf_relevel launch and a job upload per candidate; here the frames are the streams' own, held as records wherever they lie, and a
// round of the search is five launches for all jobs: k_lf_candidates, k_loopfilter_rows4, k_quality_blocks, k_quality_sum, k_lf_choose
// (lf_search_kernels.hip; the rule in lf_choose.hh).
namespace {

// One job of the call while it runs
struct LfBatchJob {
  aa_stream * s; FrameRec * r;
  size_t raster_bytes, records_off, job_off, per;     // a candidate: raster | records | job record, `per` bytes in all
  uint32_t nmb, geometry;
  aa::LfSegments seg;
  aa::LfChoice state;
  int next_level;
};

// Events of one timed section on the compute stream -> ms (0 if an event could not be had: timing is a report, not a result)
struct LfSections {
  aa_ctx * ctx; std::vector<hipEvent_t> ev;
  explicit LfSections( aa_ctx * c ) : ctx( c ) {}
  ~LfSections() { for ( hipEvent_t e : ev ) if ( e ) ctx->free_events.push_back( e ); }
  void mark() { hipEvent_t e = get_event( ctx ); if ( e ) (void) hipEventRecord( e, ctx->compute ); ev.push_back( e ); }
  // after a synchronise: ms between consecutive marks are added to out[0 .. marks - 2]; the marks are given back
  void collect( double * out )
  {
    for ( size_t i = 0; i + 1 < ev.size(); i++ ) { float ms = 0; if ( ev[i] && ev[i + 1] && hipEventElapsedTime( &ms, ev[i], ev[i + 1] ) == hipSuccess ) out[i] += ms; }
    for ( hipEvent_t e : ev ) if ( e ) ctx->free_events.push_back( e );
    ev.clear();
  }
};

// Scratch a slice may take when the caller sets no number of jobs: an eighth of the context's memory limit, at most 8 GiB (480 jobs of
// 1080p at four levels a round take 7.3 GB); a piece of that size is the device's again when the slice is over
size_t lf_slice_bytes( const aa_ctx * ctx ) { return std::min<size_t>( std::max<size_t>( ctx->pool_soft_limit / 8, size_t( 64 ) << 20 ), size_t( 8 ) << 30 ); }

} // namespace

extern "C" {

aa_status aa_ctx_set_lf_search_round( aa_ctx * ctx, int levels_per_round, int jobs_per_slice )
{
  if ( !ctx || levels_per_round < 1 || levels_per_round > AA_LF_MAX_ROUND || jobs_per_slice < 0 )
    return fail( AA_ERR_ARGUMENT, "aa_ctx_set_lf_search_round: 1..8 levels per round, 0 (by memory) or more jobs per slice" );
  ctx->lf_round = levels_per_round; ctx->lf_jobs_per_slice = jobs_per_slice;
  return AA_OK;
}

static aa_status lf_search_decode_batch( aa_ctx * ctx, aa_lf_search_job * jobs, int n, int measure );
// (every message of the call names the call: the refusals do by themselves, what a shared piece reports -- a launch, a copy, the pool,
// the watchdog -- gets the name in front here)
aa_status aa_lf_search_decode_batch( aa_ctx * ctx, aa_lf_search_job * jobs, int n, int measure )
{
  const aa_status st = lf_search_decode_batch( ctx, jobs, n, measure );
  const std::string who = "aa_lf_search_decode_batch: ";
  if ( st != AA_OK && g_last_error.compare( 0, who.size(), who ) != 0 ) g_last_error = who + g_last_error;
  return st;
}
static aa_status lf_search_decode_batch( aa_ctx * ctx, aa_lf_search_job * jobs, int n, int measure )
{
  const auto no = []( aa_status code, const std::string & what ) { return fail( code, "aa_lf_search_decode_batch: " + what ); };
  const auto no_job = [&no]( aa_status code, int i, const std::string & what ) { return no( code, "job " + std::to_string( i ) + ": " + what ); };
  // ---- 1. the arguments: nothing is decoded, no stream changed, no output written unless every job of the call is good ----
  if ( !ctx || n < 0 || ( n > 0 && !jobs ) ) return no( AA_ERR_ARGUMENT, "null pointer or a negative number of jobs" );
  if ( measure != AA_LF_MEASURE_SSIM && measure != AA_LF_MEASURE_SSE ) return no( AA_ERR_ARGUMENT, "measure is neither AA_LF_MEASURE_SSIM (0) nor AA_LF_MEASURE_SSE (1)" );
  if ( n == 0 ) return AA_OK;
  if ( aa_status st = set_device( ctx ) ) return st;
  for ( int i = 0; i < n; i++ ) {
    const aa_lf_search_job & j = jobs[i];
    if ( !j.stream || !j.original.y ) return no_job( AA_ERR_ARGUMENT, i, "null pointer" );
    aa_stream * s = j.stream;
    if ( s->ctx != ctx ) return no_job( AA_ERR_ARGUMENT, i, "stream belongs to another context" );
    for ( int k = 0; k < i; k++ ) if ( jobs[k].stream == s ) return no_job( AA_ERR_ARGUMENT, i, "its stream is also job " + std::to_string( k ) + "'s: one frame per stream and call" );
    if ( j.level_lo < 0 || j.level_hi > 63 || j.level_lo > j.level_hi ) return no_job( AA_ERR_ARGUMENT, i, "levels must be 0 <= lo <= hi <= 63" );
    if ( j.frame_index < 0 || j.frame_index >= static_cast<int>( s->frames.size() ) ) return no_job( AA_ERR_ARGUMENT, i, "frame index out of range" );
    if ( j.frame_index != s->next_submit ) return no_job( AA_ERR_LOGIC, i, "the frame is not its stream's next to decode" );
    const FrameRec & r = s->frames[j.frame_index];
    if ( r.records_released || !r.handle_held ) return no_job( AA_ERR_LOGIC, i, "the frame or its records were released" );
    if ( r.hdr.key_frame ) return no_job( AA_ERR_ARGUMENT, i, "a key frame: the search is the re-encode's, which makes inter frames" );
    if ( j.original.y_stride < int64_t( s->pw ) ) return no_job( AA_ERR_ARGUMENT, i, "row stride smaller than the padded plane's width" );
  }
  if ( ctx->schedule != 0 )
    return no( AA_ERR_UNSUPPORTED, "the diagonal schedule has no row-pipelined loop filter to launch over the candidates (aa_ctx_set_schedule( ctx, AA_SCHEDULE_ROWS ))" );

  const double t_call = now_ms();
  double timing[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
  LfSections sections( ctx );

  // ---- 2. every frame reconstructed once, unfiltered: the batch's normal launches with the loop-filter step held back ----
  std::vector<aa_stream *> streams( n );
  std::vector<int> fis( n );
  const std::vector<uint8_t> hold( n, 1 );
  for ( int i = 0; i < n; i++ ) { streams[i] = jobs[i].stream; fis[i] = jobs[i].frame_index; }
  sections.mark();
  if ( aa_status st = decode_batch_held( ctx, streams.data(), n, fis.data(), hold.data() ) ) {
    // (the shared function speaks as aa_decode_batch: the message of this call names this call)
    const std::string theirs = "aa_decode_batch: ";
    const std::string what = g_last_error.compare( 0, theirs.size(), theirs ) == 0 ? g_last_error.substr( theirs.size() ) : g_last_error;
    return no( st, "the unfiltered reconstruction: " + what );
  }
  sections.mark();

  const int K = ctx->lf_round;
  const size_t job_bytes = align_up( sizeof( aa_dev_frame ) );
  std::vector<LfBatchJob> B( n );
  int max_mbw = 0, max_mbh = 0;
  for ( int i = 0; i < n; i++ ) {
    LfBatchJob & b = B[i];
    b.s = jobs[i].stream; b.r = &b.s->frames[fis[i]];
    const aa_frame_header & h = b.r->hdr;
    b.nmb = h.num_macroblocks;
    b.geometry = ( static_cast<uint32_t>( h.mb_width ) << 16 ) | h.mb_height;
    b.raster_bytes = b.s->plane_bytes[0] + 2 * b.s->plane_bytes[1];
    b.records_off = align_up( b.raster_bytes );
    b.job_off = b.records_off + align_up( size_t( b.nmb ) * sizeof( aa_mb_info ) );
    b.per = b.job_off + job_bytes;
    // the segments' levels as the stream's DecoderState holds them -- the state itself is not touched; a frame whose header switches
    // segmentation off has one level
    const aa::SegmentationState & seg = b.s->parser.segmentation();
    b.seg = lf_segments_of( seg, h.segmentation_enabled && seg.enabled );
    aa::lf_choice_begin( b.state, jobs[i].level_lo );
    b.next_level = jobs[i].level_lo;
    max_mbw = std::max<int>( max_mbw, h.mb_width ); max_mbh = std::max<int>( max_mbh, h.mb_height );
  }
  if ( aa_status st = ensure_ws( ctx, &ctx->ws, &ctx->ws_bytes, max_mbh ) ) return st;

  // ---- 3. slice by slice, round by round ----
  const size_t share = lf_slice_bytes( ctx );
  int rounds = 0;
  for ( int first = 0; first < n; ) {
    int count = 0;
    size_t cand_total = 0;
    uint32_t max_raster = 0, max_mbs = 0;
    while ( first + count < n ) {
      const LfBatchJob & b = B[first + count];
      if ( count && ( ctx->lf_jobs_per_slice ? count >= ctx->lf_jobs_per_slice : cand_total + b.per * K > share ) ) break;
      cand_total += b.per * K;
      max_raster = std::max<uint32_t>( max_raster, static_cast<uint32_t>( b.raster_bytes ) ); max_mbs = std::max( max_mbs, b.nmb );
      count++;
    }
    // the slice's piece: job table | states (one upload, from the pinned entry's start) | round table (an upload per round) | SSIM values |
    // squared errors | the candidates.  Pinned: the same, up to the round table, then the states as they come down after every round.
    const size_t table_bytes = align_up( size_t( count ) * sizeof( aa_lf_search_dev_job ) ), states_bytes = align_up( size_t( count ) * sizeof( aa::LfChoice ) );
    const size_t entries_bytes = align_up( size_t( count ) * sizeof( aa_lf_round_entry ) ), scores_bytes = align_up( size_t( count ) * K * sizeof( double ) );
    const size_t head_bytes = table_bytes + states_bytes + entries_bytes + 2 * scores_bytes;
    const size_t piece_bytes = head_bytes + cand_total;
    JobRing::Entry * rb = nullptr;
    if ( aa_status st = ctx->lf_ring.take( table_bytes + 2 * states_bytes + entries_bytes, align_up( 64 * sizeof( aa_lf_search_dev_job ) ), &rb ) ) return st;
    uint8_t * piece = nullptr;
    if ( aa_status st = dev_alloc_compute( ctx, piece_bytes, &piece ) ) return st;
    // (the slice ends in a synchronise; a failed one waits here: a piece of gigabytes goes back to the device, dev_release_transient)
    struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { (void) hipStreamSynchronize( c->compute ); dev_release_transient( c, p, b ); } } back { ctx, piece, piece_bytes };
    const aa_lf_search_dev_job * const table_dev = reinterpret_cast<const aa_lf_search_dev_job *>( piece );
    aa::LfChoice * const states_dev = reinterpret_cast<aa::LfChoice *>( piece + table_bytes );
    aa_lf_round_entry * const entries_dev = reinterpret_cast<aa_lf_round_entry *>( piece + table_bytes + states_bytes );
    double * const ssim_dev = reinterpret_cast<double *>( piece + table_bytes + states_bytes + entries_bytes );
    uint64_t * const sse_dev = reinterpret_cast<uint64_t *>( piece + table_bytes + states_bytes + entries_bytes + scores_bytes );
    aa_lf_search_dev_job * const table = reinterpret_cast<aa_lf_search_dev_job *>( rb->host );
    aa::LfChoice * const states_up = reinterpret_cast<aa::LfChoice *>( rb->host + table_bytes );
    aa_lf_round_entry * const entries = reinterpret_cast<aa_lf_round_entry *>( rb->host + table_bytes + states_bytes );
    const aa::LfChoice * const states_down = reinterpret_cast<const aa::LfChoice *>( rb->host + table_bytes + states_bytes + entries_bytes );

    size_t cand_off = head_bytes;
    for ( int k = 0; k < count; k++ ) {
      const LfBatchJob & b = B[first + k];
      aa_lf_search_dev_job & d = table[k];
      std::memset( &d, 0, sizeof d );
      d.frame = const_cast<aa_dev_frame *>( b.r->dev_job );
      d.cand = piece + cand_off; cand_off += b.per * K;
      d.per = b.per;
      d.raster_bytes = static_cast<uint32_t>( b.raster_bytes ); d.luma_bytes = static_cast<uint32_t>( b.s->plane_bytes[0] ); d.chroma_bytes = static_cast<uint32_t>( b.s->plane_bytes[1] );
      d.records_off = static_cast<uint32_t>( b.records_off ); d.job_off = static_cast<uint32_t>( b.job_off );
      d.nmb = b.nmb; d.pw = b.s->pw; d.ph = b.s->ph;
      d.level_hi = jobs[first + k].level_hi;
      d.seg = b.seg;
      states_up[k] = b.state;
    }
    HIP_TRY( hipMemcpyAsync( piece, rb->host, table_bytes + states_bytes, hipMemcpyHostToDevice, ctx->compute ) );

    for ( ;; ) {
      // the round's table: the slice's jobs that are still searching
      int n_entries = 0; uint32_t n_scores = 0;
      std::vector<std::pair<uint32_t, const aa_dev_frame *>> keyed;
      std::vector<QualityPair> pairs;
      for ( int k = 0; k < count; k++ ) {
        const LfBatchJob & b = B[first + k];
        if ( b.state.done ) continue;
        aa_lf_round_entry & e = entries[n_entries++];
        e.job = static_cast<uint32_t>( k ); e.first_level = b.next_level;
        e.n = static_cast<uint32_t>( std::min( K, jobs[first + k].level_hi - b.next_level + 1 ) );
        e.score_off = n_scores; n_scores += e.n;
        uint8_t * const own = slot_plane( b.s, b.r->out_slot, 0 );
        const aa_quality_ref & o = jobs[first + k].original;
        for ( uint32_t c = 0; c < e.n; c++ ) {
          const int level = e.first_level + static_cast<int>( c );
          uint8_t * const cand = table[k].cand + c * b.per;
          // level 0: Frame::loopfilter does nothing (frame.cc:144) -- the unfiltered raster itself is scored
          if ( level ) keyed.emplace_back( b.geometry, reinterpret_cast<const aa_dev_frame *>( cand + b.job_off ) );
          pairs.push_back( { level ? cand : own, int64_t( b.s->pw ), static_cast<const uint8_t *>( o.y ), o.y_stride, b.s->pw, b.s->ph } );
        }
      }
      if ( !n_entries ) break;
      rounds++;
      const size_t base = sections.ev.size();      // (2 in the call's first round: the marks around the reconstruction)
      sections.mark();
      HIP_TRY( hipMemcpyAsync( entries_dev, entries, size_t( n_entries ) * sizeof( aa_lf_round_entry ), hipMemcpyHostToDevice, ctx->compute ) );
      if ( int e = aa::launch_lf_candidates( table_dev, entries_dev, n_entries, max_raster, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_lf_candidates" );
      sections.mark();
      if ( !keyed.empty() ) if ( aa_status st = launch_lf_rows( ctx, keyed, false, max_mbh, max_mbw ) ) return st;
      sections.mark();
      if ( aa_status st = quality_of_planes( ctx, pairs.data(), static_cast<int>( pairs.size() ), ssim_dev, measure == AA_LF_MEASURE_SSE ? sse_dev : nullptr, nullptr ) ) return st;
      sections.mark();
      if ( int e = aa::launch_lf_choose( table_dev, entries_dev, n_entries, ssim_dev, reinterpret_cast<const unsigned long long *>( sse_dev ), measure, states_dev, ctx->compute ) )
        return hip_fail( static_cast<hipError_t>( e ), "k_lf_choose" );
      // one small copy per round: who is done, and where everybody stands
      HIP_TRY( hipMemcpyAsync( const_cast<aa::LfChoice *>( states_down ), states_dev, size_t( count ) * sizeof( aa::LfChoice ), hipMemcpyDeviceToHost, ctx->compute ) );
      sections.mark();
      HIP_TRY( hipStreamSynchronize( ctx->compute ) );
      if ( aa_status st = check_watchdog( ctx ) ) return st;
      { double part[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }; sections.collect( part ); if ( base ) timing[1] += part[0]; for ( int k = 0; k < 4; k++ ) timing[2 + k] += part[base + k]; }
      for ( int e = 0; e < n_entries; e++ ) {
        LfBatchJob & b = B[first + entries[e].job];
        b.state = states_down[entries[e].job];
        b.next_level += static_cast<int>( entries[e].n );
      }
    }

    // ---- 4. the chosen level into every job's own records and job record, then its own raster filtered in place: the reference's last
    //         frame.loopfilter( ..., reconstructed ) ----
    sections.mark();
    if ( int e = aa::launch_lf_finish( table_dev, states_dev, count, max_mbs, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_lf_finish" );
    if ( aa_status st = ctx->lf_ring.mark( *rb, ctx->compute ) ) return st;
    std::vector<std::pair<uint32_t, const aa_dev_frame *>> keyed;
    for ( int k = 0; k < count; k++ ) if ( B[first + k].state.best_level > 0 ) keyed.emplace_back( B[first + k].geometry, B[first + k].r->dev_job );
    if ( !keyed.empty() ) if ( aa_status st = launch_lf_rows( ctx, keyed, false, max_mbh, max_mbw ) ) return st;
    sections.mark();
    HIP_TRY( hipStreamSynchronize( ctx->compute ) );
    if ( aa_status st = check_watchdog( ctx ) ) return st;
    { double part[2] = { 0, 0 }; sections.collect( part ); timing[6] += part[0]; }
    // ... and what the host holds of these frames: the stored header, and the records of frames that came from the host
    for ( int k = 0; k < count; k++ ) {
      LfBatchJob & b = B[first + k];
      FrameRec & r = *b.r;
      const int level = b.state.best_level;
      r.hdr.loop_filter_level = static_cast<uint8_t>( level );
      r.hdr.filter_adjustments_enabled = 1;
      if ( r.host_job ) {
        r.host_job->loop_filter_level = static_cast<uint8_t>( level );
        const uint32_t levels = aa::lf_segment_levels( b.seg, level );
        aa_mb_info * mbs = reinterpret_cast<aa_mb_info *>( reinterpret_cast<uint8_t *>( r.host_job ) + job_bytes );
        for ( uint32_t m = 0; m < b.nmb; m++ ) mbs[m].lf_level = static_cast<uint8_t>( ( levels >> ( 8 * ( mbs[m].segment_id & 3 ) ) ) & 255u );
      }
    }
    first += count;
  }

  for ( int i = 0; i < n; i++ ) { jobs[i].best_level = B[i].state.best_level; jobs[i].evaluated = B[i].state.evaluated; jobs[i].best_score = B[i].state.best_score; }
  timing[0] = now_ms() - t_call; timing[7] = rounds;
  std::memcpy( ctx->lf_timing, timing, sizeof timing );
  return AA_OK;
}

aa_status aa_lf_search_last_timing( aa_ctx * ctx, double out[8] )
{
  if ( !ctx || !out ) return fail( AA_ERR_ARGUMENT, "aa_lf_search_last_timing: null argument" );
  std::memcpy( out, ctx->lf_timing, sizeof ctx->lf_timing );
  return AA_OK;
}

} // extern "C"
