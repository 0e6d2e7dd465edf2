// runtime.cpp, one of its pieces (ABI): frames going to reconstruction -- parse summaries, aa_stream_read_records, the row kernels' launches,
// aa_decode_batch, release / rewind.
extern "C" {

// counts the device parser produced (intra macroblocks, coefficient blocks, SPLITMV) -> the frame's header; waits for the parse
static aa_status resolve_summary( aa_stream * s, FrameRec & r )
{
  if ( !r.summary_pending ) return AA_OK;
  aa_ctx * ctx = s->ctx;
  auto & T = ctx->tok;
  Batch * b = r.batch;
  if ( !b || !r.summary ) return fail( AA_ERR_LOGIC, "frame records were released before the frame was decoded" );
  if ( b->tokens_pending ) if ( aa_status st = launch_tokens_of( ctx, b ) ) return st;      // two-phase submit, second phase not asked for yet
  volatile aa::FrameSummary * sum = r.summary;
  for ( int attempt = 0; ; attempt++ ) {
    if ( aa_status st = tok_wait_done( ctx, sum ) ) return st;
    if ( sum->status != aa::TOK_NO_MEMORY ) break;
    // The coefficient pool ran dry under this frame's lane and nothing came back in time: the lane handed the frame back.  Its
    // chunks are returned, room is made (more heap if the memory limit allows it, else by letting everything else in flight
    // finish) and the frame goes to the queue again -- its macroblock headers are parsed already.
    ctx->stats.nomem_retries++;
    const uint32_t worst = aa::chunk_list_entries( r.hdr.num_macroblocks, T.lane_per_partition ? 8u : 1u );      // (what no frame of this size exceeds, in either storage format)
    {
      std::lock_guard<std::mutex> g( ctx->pool_mu );
      // (marked as returned at once: a call that fails below and is repeated must not push the list a second time)
      if ( !r.chunks_returned ) { T.pending_lists.push_back( r.chunk_list ); r.chunks_returned = true; T.chunks_committed -= r.est_chunks; r.est_chunks = 0; }
      flush_chunk_frees( ctx );                     // (and the chunks of everything the caller has released since)
      if ( !T.pending_lists.empty() ) return fail( AA_ERR_HIP, "k_pool_free_lists could not be launched" );
    }
    HIP_TRY( hipStreamSynchronize( ctx->compute ) );
    if ( aa_status st = tok_grow_heap( ctx, T.heap_mapped + static_cast<size_t>( worst ) * kChunkBytesHeap ) ) return st;
    if ( aa_status st = tok_refresh_mirror( ctx ) ) return st;
    if ( T.mirror_host->pool_avail < static_cast<int32_t>( worst ) ) {
      if ( aa_status st = tok_quiesce( ctx ) ) return st;
      if ( aa_status st = tok_refresh_mirror( ctx ) ) return st;
    }
    if ( T.mirror_host->pool_avail < static_cast<int32_t>( worst ) ) {
      // Still not enough: the heap is held by frames that were parsed AHEAD of this one (submitted later, needed later).  They
      // give their chunks back -- newest first -- and are parsed again when their turn comes: to them it is as if their lane had
      // handed them back.  Thrashing is slow, but a caller that looks far ahead never gets stuck on the frame it needs now.
      int32_t have = T.mirror_host->pool_avail;
      std::lock_guard<std::mutex> g( ctx->pool_mu );
      for ( auto bi = T.batches.rbegin(); bi != T.batches.rend() && have < static_cast<int32_t>( worst ); ++bi ) {
        Batch * vb = *bi;
        volatile aa::FrameSummary * sums = reinterpret_cast<volatile aa::FrameSummary *>( vb->host + vb->summaries_off );
        for ( int i = vb->n - 1; i >= 0 && have < static_cast<int32_t>( worst ); i-- ) {
          if ( !vb->items[i].live ) continue;
          aa_stream * vs = vb->items[i].s;
          FrameRec & v = vs->frames[vb->items[i].frame];
          if ( &v == &r || vb->items[i].on_host || !v.enqueued || v.records_released || v.chunks_returned || !sums[i].done || vb->items[i].frame < vs->next_submit ) continue;     // (a host lane's frame holds no chunks)
          T.pending_lists.push_back( v.chunk_list );
          have += static_cast<int32_t>( sums[i].num_chunks );
          v.chunks_returned = true; v.summary_pending = true;
          T.chunks_committed -= v.est_chunks; v.est_chunks = 0;
          sums[i].status = aa::TOK_NO_MEMORY;
          ctx->stats.frames_evicted++;
        }
      }
      flush_chunk_frees( ctx );
      if ( !T.pending_lists.empty() ) return fail( AA_ERR_HIP, "k_pool_free_lists could not be launched" );
    }
    HIP_TRY( hipStreamSynchronize( ctx->compute ) );
    if ( aa_status st = tok_refresh_mirror( ctx ) ) return st;
    if ( attempt >= 8 || T.mirror_host->pool_avail < static_cast<int32_t>( worst ) )
      return fail( AA_ERR_NO_MEMORY, "device parser: the coefficient heap is exhausted (" + std::to_string( T.heap_mapped >> 20 ) + " MiB mapped, "
                                     + std::to_string( T.mirror_host->pool_avail ) + " chunks free, this frame may need " + std::to_string( worst )
                                     + "): release decoded frames (aa_stream_release_before) or raise the limit (aa_ctx_set_memory_limit); the call can be repeated" );
    sum->status = 0; sum->done = 0; sum->num_chunks = 0;
    r.chunks_returned = false;
    r.est_chunks = worst; T.chunks_committed += worst;
    __atomic_thread_fence( __ATOMIC_SEQ_CST );
    if ( int e = aa::launch_enqueue_jobs( T.q, T.slots, r.parse_job, T.one_dev, 1, T.util ) ) return hip_fail( static_cast<hipError_t>( e ), "k_enqueue_jobs" );
    T.jobs_enqueued += 1;
    if ( std::find( T.inflight.begin(), T.inflight.end(), b ) == T.inflight.end() ) T.inflight.push_back( b );
    if ( aa_status st = tok_service( ctx ) ) return st;
  }
  if ( sum->status == aa::TOK_HOST_FAILED ) return fail( AA_ERR_HIP, "host lane: the frame's records could not be placed in device memory" );
  if ( sum->status == aa::TOK_STEP_BOUND ) return fail( AA_ERR_HIP, "device parser: a token lane exceeded the step bound of its frame size (records are not valid)" );
  r.hdr.num_coeff_blocks = sum->num_coeff_blocks;
  r.hdr.num_intra_mbs = sum->num_intra_mbs;
  r.hdr.has_intra_mb = sum->num_intra_mbs != 0;
  r.has_split = sum->has_split != 0;
  r.intra_diagonals.assign( r.hdr.mb_width + 2 * ( r.hdr.mb_height - 1 ), r.hdr.has_intra_mb ? 1 : 0 );   // diagonal schedule: all of them
  // the books: what the frame really took; what macroblocks store on this content (feeds the estimate of later frames)
  T.chunks_committed += static_cast<int64_t>( sum->num_chunks ) - static_cast<int64_t>( r.est_chunks );
  r.est_chunks = sum->num_chunks;
  if ( r.hdr.compressed_size ) T.blocks_per_byte += 0.05 * ( static_cast<double>( sum->num_coeff_blocks ) / r.hdr.compressed_size - T.blocks_per_byte );
  if ( r.hdr.compressed_size && r.packed_pos ) T.words_per_byte += 0.05 * ( static_cast<double>( sum->packed_words ) / r.hdr.compressed_size - T.words_per_byte );
  if ( r.packed_pos ) { ctx->stats.packed_frames++; ctx->stats.packed_words += sum->packed_words; ctx->stats.packed_blocks += sum->num_coeff_blocks; }
  ctx->stats.token_steps += sum->steps; ctx->stats.token_frames++;
  r.summary_pending = false;
  return AA_OK;
}

aa_status aa_stream_frame_header( aa_stream * s, int fi, aa_frame_header * out )
{
  if ( !s || !out || fi < 0 || fi >= static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_ARGUMENT, "aa_stream_frame_header: bad argument" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  if ( aa_status st = resolve_summary( s, s->frames[fi] ) ) return st;
  *out = s->frames[fi].hdr;
  return AA_OK;
}

/* Debug / test view of a frame's parsed records as they sit in HBM (host- or device-parsed alike). */
aa_status aa_stream_read_records( aa_stream * s, int fi, aa_mb_info * mb_out, int16_t * coeff_out, size_t coeff_capacity_blocks )
{
  if ( !s || fi < 0 || fi >= static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_ARGUMENT, "aa_stream_read_records: bad argument" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  FrameRec & r = s->frames[fi];
  if ( r.records_released ) return fail( AA_ERR_LOGIC, "aa_stream_read_records: frame records were released" );
  if ( aa_status st = resolve_summary( s, r ) ) return st;
  if ( aa_status st = aa_stream_upload( s ) ) return st;
  HIP_TRY( hipStreamSynchronize( s->ctx->copy ) );        // (also covers the arena of a host-parsed submit call: same stream)
  aa_dev_frame job;
  HIP_TRY( hipMemcpy( &job, r.dev_job, sizeof job, hipMemcpyDeviceToHost ) );
  if ( coeff_out && coeff_capacity_blocks < r.hdr.num_coeff_blocks ) return fail( AA_ERR_ARGUMENT, "aa_stream_read_records: coefficient buffer too small" );
  if ( !r.chunk_list ) {                     // host-parsed: the blocks follow each other in the frame-store chunk
    if ( mb_out ) HIP_TRY( hipMemcpy( mb_out, job.mbs, size_t( r.hdr.num_macroblocks ) * sizeof( aa_mb_info ), hipMemcpyDeviceToHost ) );
    if ( coeff_out ) HIP_TRY( hipMemcpy( coeff_out, job.coeffs, size_t( r.hdr.num_coeff_blocks ) * 32, hipMemcpyDeviceToHost ) );
    return AA_OK;
  }
  // device-parsed: the blocks sit in chunks of the coefficient heap and coeff_index is a heap index.  The caller gets the
  // frame's own view -- blocks back to back in parse order, coeff_index counted from the frame's first block -- which is
  // what the host parser produces.
  std::vector<aa_mb_info> mbs( r.hdr.num_macroblocks );
  HIP_TRY( hipMemcpy( mbs.data(), job.mbs, mbs.size() * sizeof( aa_mb_info ), hipMemcpyDeviceToHost ) );
  std::vector<uint32_t> list( size_t( r.est_chunks ) + 1 );
  HIP_TRY( hipMemcpy( list.data(), r.chunk_list, list.size() * sizeof( uint32_t ), hipMemcpyDeviceToHost ) );
  if ( list[0] != r.est_chunks ) return fail( AA_ERR_LOGIC, "aa_stream_read_records: chunk list disagrees with the parse summary" );
  if ( r.packed_pos ) {
    // packed storage: the frame's words are expanded here as k_dense_index / k_expand_coeffs do it on the device (coeff_pack.hh)
    std::vector<uint32_t> pos( r.hdr.num_macroblocks );
    HIP_TRY( hipMemcpy( pos.data(), r.packed_pos, pos.size() * sizeof( uint32_t ), hipMemcpyDeviceToHost ) );
    std::vector<std::vector<int16_t>> words( list[0] );
    if ( coeff_out )
      for ( uint32_t k = 0; k < list[0]; k++ ) {
        words[k].resize( aa::kChunkWords );
        HIP_TRY( hipMemcpy( words[k].data(), s->ctx->tok.heap + size_t( list[1 + k] ) * kChunkBytesHeap, kChunkBytesHeap, hipMemcpyDeviceToHost ) );
      }
    uint32_t running = 0;
    for ( size_t mi = 0; mi < mbs.size(); mi++ ) {
      aa_mb_info & mb = mbs[mi];
      const uint32_t nblk = aa::pack::blocks_of( mb.nz_mask );
      if ( nblk && coeff_out ) {
        const uint32_t ord = pos[mi] >> 15, off = pos[mi] & ( aa::kChunkWords - 1u );
        if ( ord >= list[0] || running + nblk > r.hdr.num_coeff_blocks )
          return fail( AA_ERR_LOGIC, "aa_stream_read_records: a macroblock's coefficients lie outside the frame's chunks" );
        // (a macroblock's words end inside its chunk -- the lane made sure of it; checked all the same: the mask slots, then the
        // values its masks announce)
        const int16_t * w = words[ord].data() + off, * end = words[ord].data() + aa::kChunkWords;
        if ( w + aa::pack::kMaskSlots > end ) return fail( AA_ERR_LOGIC, "aa_stream_read_records: packed coefficients run past their chunk" );
        uint32_t values = 0;
        for ( uint32_t b = 0; b < 25; b++ ) if ( ( mb.nz_mask >> b ) & 1u ) values += aa::pack::popc( static_cast<uint16_t>( w[b] ) );
        if ( w + aa::pack::kMaskSlots + values > end ) return fail( AA_ERR_LOGIC, "aa_stream_read_records: packed coefficients run past their chunk" );
        // (the record's own offset -- what the reconstruction kernels follow -- must name the same words)
        if ( ( static_cast<unsigned long long>( mb.reserved ) << 32 | mb.coeff_index ) != static_cast<unsigned long long>( list[1 + ord] ) * aa::kChunkWords + off )
          return fail( AA_ERR_LOGIC, "aa_stream_read_records: a macroblock's word offset disagrees with its place in the frame's chunks" );
        aa::pack::expand_macroblock( w, mb.nz_mask, coeff_out + size_t( running ) * 16 );
      }
      mb.coeff_index = running; mb.reserved = 0;
      running += nblk;
    }
    if ( running != r.hdr.num_coeff_blocks ) return fail( AA_ERR_LOGIC, "aa_stream_read_records: non-zero masks disagree with the parse summary" );
    if ( mb_out ) std::memcpy( mb_out, mbs.data(), mbs.size() * sizeof( aa_mb_info ) );
    return AA_OK;
  }
  std::map<uint32_t, std::vector<uint8_t>> chunk;
  if ( coeff_out )
    for ( uint32_t k = 0; k < list[0]; k++ ) {
      auto & v = chunk[list[1 + k]];
      v.resize( kChunkBytesHeap );
      HIP_TRY( hipMemcpy( v.data(), s->ctx->tok.heap + size_t( list[1 + k] ) * kChunkBytesHeap, kChunkBytesHeap, hipMemcpyDeviceToHost ) );
    }
  uint32_t running = 0;
  for ( auto & mb : mbs ) {
    const uint32_t nblk = static_cast<uint32_t>( __builtin_popcount( mb.nz_mask ) );
    if ( nblk && coeff_out ) {
      auto it = chunk.find( mb.coeff_index / aa::kChunkBlocks );
      if ( it == chunk.end() || mb.coeff_index % aa::kChunkBlocks + nblk > aa::kChunkBlocks || running + nblk > r.hdr.num_coeff_blocks )
        return fail( AA_ERR_LOGIC, "aa_stream_read_records: a macroblock's coefficients lie outside the frame's chunks" );
      std::memcpy( coeff_out + size_t( running ) * 16, it->second.data() + size_t( mb.coeff_index % aa::kChunkBlocks ) * 32, size_t( nblk ) * 32 );
    }
    mb.coeff_index = running;
    running += nblk;
  }
  if ( running != r.hdr.num_coeff_blocks ) return fail( AA_ERR_LOGIC, "aa_stream_read_records: non-zero masks disagree with the parse summary" );
  if ( mb_out ) std::memcpy( mb_out, mbs.data(), mbs.size() * sizeof( aa_mb_info ) );
  return AA_OK;
}

namespace {
// Row-pipelined loop filter over a set of frames: four frames of ONE geometry per wave.  Bucket by geometry, pad every bucket
// to a multiple of four with null frames (slot 0 of a group is never null), split at group boundaries when a list is full.
aa_status launch_lf_rows( aa_ctx * ctx, std::vector<std::pair<uint32_t, const aa_dev_frame *>> & keyed, bool same_geometry, int max_mbh, int max_mbw )
{
  if ( !same_geometry ) std::stable_sort( keyed.begin(), keyed.end(), []( const auto & a, const auto & b ) { return a.first < b.first; } );
  aa_frame_list list;
  int filled = 0;
  auto launch = [&]() -> aa_status {
    if ( !filled ) return AA_OK;
    for ( int k = filled; k < AA_MAX_BATCH; k++ ) list.f[k] = nullptr;
    if ( aa_status st = zero_ws( ctx, ctx->ws, filled / 4, max_mbh ) ) return st;
    const size_t need = size_t( filled ) * max_mbh * max_mbw * 128;
    if ( need > ctx->boundary_bytes ) {
      HIP_TRY( hipStreamSynchronize( ctx->compute ) );
      if ( ctx->boundary ) (void) hipFree( ctx->boundary );
      ctx->boundary = nullptr; ctx->boundary_bytes = 0;
      HIP_TRY( hipMalloc( reinterpret_cast<void **>( &ctx->boundary ), need ) );
      ctx->boundary_bytes = need;
    }
    LaunchTimer t( ctx, 2 );
    if ( const int e = aa::launch_loopfilter_rows4( list, filled / 4, max_mbh, max_mbw, ctx->ws, ctx->boundary, ctx->n_xcd, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_loopfilter_rows4" );
    filled = 0;
    return AA_OK;
  };
  for ( size_t i = 0; i < keyed.size(); ) {
    size_t j = i;
    while ( j < keyed.size() && j - i < 4 && keyed[j].first == keyed[i].first ) j++;
    for ( size_t k = 0; k < 4; k++ ) list.f[filled++] = i + k < j ? keyed[i + k].second : nullptr;
    i = j;
    if ( filled + 4 > AA_MAX_BATCH ) if ( aa_status st = launch() ) return st;
  }
  return launch();
}
} // namespace

namespace {
// ALFALFA_AMD_DECODE_TIMING=1 (diagnostics, off by default): where the host's time inside aa_decode_batch goes, section by section, printed
// to stderr when a context is destroyed.  (Round 5: the plateau's calls take 24 ms each with the counted waits at zero, DESIGN.md section 8.)
struct DecodeTiming {
  bool on = false; double ms[10] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }; uint64_t calls = 0;
  ~DecodeTiming()      // (the static below: at process exit)
  {
    if ( !on || !calls ) return;
    static const char * const names[10] = { "checks", "stream uploads", "collect_pending", "resolve_summary (waits for the parser included)", "dense buffer",
                                            "bind_batch (waits for a binding buffer included)", "expand_packed", "job lists", "inter launches", "intra + loop-filter launches" };
    std::fprintf( stderr, "alfalfa_amd: aa_decode_batch host time over %llu calls, ms per call:", static_cast<unsigned long long>( calls ) );
    for ( int k = 0; k < 10; k++ ) std::fprintf( stderr, " [%s] %.3f", names[k], ms[k] / static_cast<double>( calls ) );
    std::fprintf( stderr, "\n" );
  }
};
DecodeTiming * decode_timing() { static DecodeTiming d; static const bool init = [] { const char * e = std::getenv( "ALFALFA_AMD_DECODE_TIMING" ); d.on = e && atoi( e ) != 0; return true; }(); (void) init; return &d; }
struct DecodeMark {
  DecodeTiming & d; double t;
  DecodeMark() : d( *decode_timing() ), t( d.on ? now_ms() : 0.0 ) { if ( d.on ) d.calls++; }
  void lap( int k ) { if ( d.on ) { const double n = now_ms(); d.ms[k] += n - t; t = n; } }
};
} // namespace

// aa_decode_batch.  hold_filter (null: nobody's): frame i with hold_filter[i] set is reconstructed but NOT loop-filtered -- its level is
// still being searched (aa_lf_search_decode_batch, which filters it in place once the level is known); everything else of the frame's
// decode -- raster, References, next_submit -- is done as for any frame.
static aa_status decode_batch_held( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index, const uint8_t * hold_filter )
{
  if ( !ctx || !streams || !frame_index || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_decode_batch: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  std::vector<const aa_dev_frame *> inter_jobs, intra_jobs, lf_jobs;
  std::vector<const FrameRec *> intra_recs;
  std::vector<uint32_t> lf_geometry;
  unsigned max_mbs = 0; int max_mbw = 0, max_mbh = 0;
  bool any_split = false;
  bool same_geometry = true;     // two-frames-per-wave loop filter needs equal macroblock dimensions in the batch
  uint64_t total_mbs = 0;
  DecodeMark mk;
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = streams[i];
    if ( !s || s->ctx != ctx ) return fail( AA_ERR_ARGUMENT, "aa_decode_batch: stream belongs to another context" );
    const int fi = frame_index[i];
    if ( fi < 0 || fi >= static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_ARGUMENT, "aa_decode_batch: frame index out of range" );
    if ( fi != s->next_submit ) return fail( AA_ERR_LOGIC, "aa_decode_batch: frames of a stream must be submitted in order" );
  }
  mk.lap( 0 );
  for ( int i = 0; i < n; i++ ) if ( aa_status st = aa_stream_upload( streams[i] ) ) return st;
  mk.lap( 1 );
  // coefficient chunks of the frames released since the last call go back to the pool (behind the kernels that read them:
  // those were queued before the release)
  // ... and what was released since then gets its epoch now: reusable as soon as the kernels queued before this call have run
  // (not whenever some later allocation happens to miss its free list)
  { std::lock_guard<std::mutex> g( ctx->pool_mu ); collect_pending( ctx, false ); }
  mk.lap( 2 );
  for ( int i = 0; i < n; i++ ) {
    if ( streams[i]->frames[frame_index[i]].records_released ) return fail( AA_ERR_LOGIC, "aa_decode_batch: frame records were released" );
    if ( aa_status st = resolve_summary( streams[i], streams[i]->frames[frame_index[i]] ) ) return st;
  }
  mk.lap( 3 );
  // (packed coefficient storage: the reconstruction kernels read the packed words themselves -- kernels.hip, residual_x4 -- since
  // round 6; rounds 3-5 expanded every frame of the call into a transient dense array here: k_dense_index + k_expand_coeffs, a
  // quarter of the reconstruction's GPU time and 972 bytes of HBM traffic per macroblock)
  // rasters released while binding (old references, outputs nobody holds) must not be recycled before this call's kernels
  // are queued: no release epoch is closed until then
  struct BindGuard { aa_ctx * c;
                     explicit BindGuard( aa_ctx * x ) : c( x ) { std::lock_guard<std::mutex> g( c->pool_mu ); c->binding_depth++; }
                     ~BindGuard() {
                       std::lock_guard<std::mutex> g( c->pool_mu );
                       if ( --c->binding_depth == 0 ) {      // every launch of the call is queued (or the call failed before any): what it released may be handed out
                         for ( auto & h : c->compute_hold ) { c->compute_free[h.second].push_back( h.first ); c->compute_free_bytes += h.second; }
                         c->compute_hold.clear();
                       } } } bind_guard( ctx );
  mk.lap( 4 );
  if ( aa_status st = bind_batch( ctx, streams, n, frame_index ) ) return st;
  mk.lap( 5 );
  // frames count as submitted only once every launch of the batch has been queued (a failed launch must not leave them
  // looking decoded)
  struct Advance { aa_stream * const * streams; int n; bool ok = false; ~Advance() { if ( ok ) for ( int i = 0; i < n; i++ ) streams[i]->next_submit++; } } advance { streams, n };
  mk.lap( 6 );
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = streams[i];
    const FrameRec & r = s->frames[frame_index[i]];
    const aa_frame_header & h = r.hdr;
    if ( h.num_intra_mbs < h.num_macroblocks ) { inter_jobs.push_back( r.dev_job ); any_split = any_split || r.has_split; }
    if ( h.has_intra_mb ) { intra_jobs.push_back( r.dev_job ); intra_recs.push_back( &r ); }
    if ( h.loop_filter_level && !( hold_filter && hold_filter[i] ) ) { lf_jobs.push_back( r.dev_job ); lf_geometry.push_back( ( static_cast<uint32_t>( h.mb_width ) << 16 ) | h.mb_height ); }
    if ( i > 0 && ( h.mb_width != streams[0]->frames[frame_index[0]].hdr.mb_width || h.mb_height != streams[0]->frames[frame_index[0]].hdr.mb_height ) ) same_geometry = false;
    max_mbs = std::max<unsigned>( max_mbs, h.num_macroblocks );
    max_mbw = std::max<int>( max_mbw, h.mb_width ); max_mbh = std::max<int>( max_mbh, h.mb_height );
    total_mbs += h.num_macroblocks;
  }
  ctx->stats.macroblocks += total_mbs;
  mk.lap( 7 );

  auto for_each_list = [&]( const std::vector<const aa_dev_frame *> & jobs, auto && fn ) -> int {
    for ( size_t base = 0; base < jobs.size(); base += AA_MAX_BATCH ) {
      aa_frame_list list;
      const int cnt = static_cast<int>( std::min<size_t>( AA_MAX_BATCH, jobs.size() - base ) );
      for ( int k = 0; k < cnt; k++ ) list.f[k] = jobs[base + k];
      for ( int k = cnt; k < AA_MAX_BATCH; k++ ) list.f[k] = nullptr;
      if ( int e = fn( list, cnt ) ) return e;
    }
    return 0;
  };
  auto check = [&]( int e, const char * what ) -> aa_status {
    if ( e ) return hip_fail( static_cast<hipError_t>( e ), what );
    return AA_OK;
  };

  // 1. every inter-coded macroblock of the batch: whole-vector macroblocks four per wave; SPLITMV ones (if any) one per wave
  if ( !inter_jobs.empty() ) {
    int e = for_each_list( inter_jobs, [&]( const aa_frame_list & l, int cnt ) {
      LaunchTimer t( ctx, 0 ); return aa::launch_recon_inter4( l, cnt, max_mbs, ctx->compute ); } );
    if ( aa_status st = check( e, "k_recon_inter4" ) ) return st;
    if ( any_split ) {
      e = for_each_list( inter_jobs, [&]( const aa_frame_list & l, int cnt ) {
        LaunchTimer t( ctx, 5 ); return aa::launch_recon_inter( l, cnt, max_mbs, true, ctx->compute ); } );
      if ( aa_status st = check( e, "k_recon_inter" ) ) return st;
    }
  }
  mk.lap( 8 );
  const int ndiag = max_mbw + 2 * ( max_mbh - 1 );
  if ( ctx->schedule == 0 ) {
    // 2+3. row-pipelined kernels: one launch each; macroblock rows are ordered in-launch (ticket + progress words)
    if ( aa_status st = ensure_ws( ctx, &ctx->ws, &ctx->ws_bytes, max_mbh ) ) return st;
    // intra rows: four frames per wave (any geometry), groups padded with null frames
    for ( size_t base = 0; base < intra_jobs.size(); base += AA_MAX_BATCH ) {
      aa_frame_list list;
      const int cnt = static_cast<int>( std::min<size_t>( AA_MAX_BATCH, intra_jobs.size() - base ) );
      const int groups = ( cnt + 3 ) / 4;
      for ( int k = 0; k < AA_MAX_BATCH; k++ ) list.f[k] = k < cnt ? intra_jobs[base + k] : nullptr;
      if ( aa_status st = zero_ws( ctx, ctx->ws, groups * 4, max_mbh ) ) return st;
      LaunchTimer t( ctx, 1 );
      if ( const int e = aa::launch_recon_intra4( list, groups, max_mbh, ctx->ws, ctx->n_xcd, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_recon_intra4" );
    }
    if ( !lf_jobs.empty() ) {
      std::vector<std::pair<uint32_t, const aa_dev_frame *>> keyed;
      keyed.reserve( lf_geometry.size() );
      for ( size_t i = 0; i < lf_jobs.size(); i++ ) keyed.emplace_back( lf_geometry[i], lf_jobs[i] );
      if ( aa_status st = launch_lf_rows( ctx, keyed, same_geometry, max_mbh, max_mbw ) ) return st;
    }
    mk.lap( 9 );
    advance.ok = true;
    return AA_OK;
  }
  // ---- ALFALFA_AMD_SCHEDULE=diagonal: the kernel boundary is the inter-workgroup synchronisation ----
  // 2. intra macroblocks, 2:1 anti-diagonal order (left, above-left, above, above-right are final)
  if ( !intra_jobs.empty() ) {
    for ( int d = 0; d < ndiag; d++ ) {
      bool needed = false;
      for ( const FrameRec * r : intra_recs ) if ( d < static_cast<int>( r->intra_diagonals.size() ) && r->intra_diagonals[d] ) { needed = true; break; }
      if ( !needed ) continue;
      const int row_lo = std::max( 0, ( d - ( max_mbw - 1 ) + 1 ) / 2 ), row_hi = std::min( max_mbh - 1, d / 2 );
      if ( row_hi < row_lo ) continue;
      const int e = for_each_list( intra_jobs, [&]( const aa_frame_list & l, int cnt ) {
        LaunchTimer t( ctx, 1 ); return aa::launch_recon_intra_diagonal( l, cnt, d, row_lo, row_hi - row_lo + 1, ctx->compute ); } );
      if ( aa_status st = check( e, "k_recon_intra" ) ) return st;
    }
  }
  // 3. loop filter over the fully reconstructed frames, same diagonal order (loopfilter.cc:133-154 dependencies)
  if ( !lf_jobs.empty() ) {
    for ( int d = 0; d < ndiag; d++ ) {
      const int row_lo = std::max( 0, ( d - ( max_mbw - 1 ) + 1 ) / 2 ), row_hi = std::min( max_mbh - 1, d / 2 );
      if ( row_hi < row_lo ) continue;
      const int e = for_each_list( lf_jobs, [&]( const aa_frame_list & l, int cnt ) {
        LaunchTimer t( ctx, 2 ); return aa::launch_loopfilter_diagonal( l, cnt, d, row_lo, row_hi - row_lo + 1, ctx->compute ); } );
      if ( aa_status st = check( e, "k_loopfilter" ) ) return st;
    }
  }
  advance.ok = true;
  return AA_OK;
}

aa_status aa_decode_batch( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index )
{
  return decode_batch_held( ctx, streams, n, frame_index, nullptr );
}

aa_status aa_stream_decode( aa_stream * s, const uint8_t * data, size_t size, int * frame_index, int * shown )
{
  int fi = -1; aa_frame_header h;
  if ( aa_status st = aa_stream_parse( s, data, size, &fi, &h ) ) return st;
  aa_stream * one[1] = { s };
  if ( aa_status st = aa_decode_batch( s->ctx, one, 1, &fi ) ) return st;
  if ( frame_index ) *frame_index = fi;
  if ( shown ) *shown = h.show_frame;
  return AA_OK;
}

int aa_stream_frame_count( const aa_stream * s ) { return s ? static_cast<int>( s->frames.size() ) : 0; }

aa_status aa_stream_set_error_concealment( aa_stream * s, int on )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  s->parser.set_error_concealment( on != 0 );       // (the host parser and the header pre-pass of the device parser: one Parser)
  return AA_OK;
}
int aa_stream_error_concealment( const aa_stream * s ) { return s && s->parser.error_concealment() ? 1 : 0; }

aa_status aa_stream_release_before( aa_stream * s, int first_kept )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  const int n = std::min<int>( first_kept, static_cast<int>( s->frames.size() ) );
  for ( int i = s->first_live; i < n; i++ ) {
    FrameRec & f = s->frames[i];
    if ( f.handle_held ) { f.handle_held = false; if ( f.placed ) release( s, f.out_slot ); }
    if ( i < s->next_submit ) release_records( s, f, true );       // decoded: nothing will read its records again once queued kernels ran
    std::vector<uint8_t>().swap( f.intra_diagonals );
  }
  while ( s->first_live < n && s->frames[s->first_live].records_released ) s->first_live++;
  return AA_OK;
}

aa_status aa_stream_rewind( aa_stream * s )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  for ( const auto & f : s->frames ) if ( !f.handle_held || f.records_released ) return fail( AA_ERR_LOGIC, "aa_stream_rewind: frames were released; slots may have been reused" );
  s->next_submit = 0;
  return AA_OK;
}

aa_status aa_stream_rewind_to( aa_stream * s, int fi )
{
  if ( !s || fi < 0 || fi > static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_ARGUMENT, "aa_stream_rewind_to: bad argument" );
  if ( fi > s->next_submit ) return fail( AA_ERR_LOGIC, "aa_stream_rewind_to: that frame has not been decoded yet" );
  for ( size_t i = fi; i < s->frames.size(); i++ )
    if ( !s->frames[i].handle_held || s->frames[i].records_released ) return fail( AA_ERR_LOGIC, "aa_stream_rewind_to: frames were released; slots may have been reused" );
  if ( fi < static_cast<int>( s->frames.size() ) && fi > 0 && !s->frames[fi].hdr.key_frame )
    for ( int r : s->frames[fi - 1].ref_after )
      if ( r < 0 || !s->frames[r].handle_held ) return fail( AA_ERR_LOGIC, "aa_stream_rewind_to: a raster that frame predicts from was released" );
  s->next_submit = fi;
  return AA_OK;
}
} // extern "C"
