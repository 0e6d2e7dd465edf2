// runtime.cpp, one of its pieces: a frame's records and rasters -- release, pinned staging, job records, References bookkeeping (bind_frame).

static uint8_t * slot_plane( aa_stream * s, int slot, int plane )
{
  uint8_t * p = s->slots[slot].dev;
  if ( plane >= 1 ) p += s->plane_bytes[0];
  if ( plane >= 2 ) p += s->plane_bytes[1];
  return p;
}

namespace {

// Give a frame's records back (device-parsed: its record block and its share of the batch arena; host-parsed: its share of
// a frame-store chunk, freed when the chunk's last frame goes).  `deferred`: queued kernels may still read them.
void release_records( aa_stream * s, FrameRec & f, bool deferred )
{
  if ( f.records_released ) return;
  aa_ctx * ctx = s->ctx;
  // a token lane may still be writing this frame's records (callers release decoded frames: then this is over already)
  bool parsed = false;
  if ( f.enqueued && f.summary ) parsed = tok_wait_done( ctx, f.summary ) == AA_OK;
  if ( !parsed && f.enqueued && f.summary && f.batch && f.batch_item >= 0 && f.batch_item < static_cast<int>( f.batch->items.size() ) && f.batch->items[f.batch_item].on_host ) {
    // A HOST LANE's frame whose wait failed (the parse timeout, or a HIP error out of the service call): a worker thread may be
    // inside host_lane_run for it right now -- reading the pinned arena, writing host_dense, queueing copies into the record
    // block -- or have it in its queue.  Nothing of the batch may be freed under it (ADVICE round 5: use-after-free, another
    // batch's records silently overwritten).  A host lane ends every path with the `done` word, so wait for that word itself,
    // without a bound and without the device.
    while ( !summary_done( f.summary ) ) usleep( 200 );
  }
  f.records_released = true;
  if ( f.rec_block ) {
    // the coefficient chunks the frame took go back to the pool on the device, by a kernel that reads the list out of the
    // record block: the block itself is recycled only behind that kernel (always through an epoch, never at once)
    const bool has_chunks = parsed && f.chunk_list && !f.chunks_returned;
    // (the list is handed to k_pool_free_lists when the open epoch is closed: mark the epoch as used, or -- with every record
    // block inside its batch arena, no deferred free of its own -- nothing would ever close it and the chunks would stay out)
    if ( has_chunks ) { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->tok.pending_lists.push_back( f.chunk_list ); ctx->open_epoch_used = true; f.chunks_returned = true; }
    if ( !f.rec_in_arena ) dev_free( ctx, f.rec_block, f.rec_bytes, deferred || has_chunks );
    f.rec_block = nullptr; f.chunk_list = nullptr; f.packed_pos = nullptr;
    ctx->tok.chunks_committed -= f.est_chunks; f.est_chunks = 0;
  }
  if ( Batch * b = f.batch ) {
    if ( f.batch_item >= 0 && f.batch_item < static_cast<int>( b->items.size() ) ) {
      Batch::Item & bi = b->items[f.batch_item];          // (a host lane's frame: its dense blocks; the wait above saw its `done` word)
      if ( bi.host_dense ) { dev_free( ctx, bi.host_dense, bi.host_dense_bytes, true ); bi.host_dense = nullptr; }
    }
    bool last;
    { std::lock_guard<std::mutex> g( ctx->pool_mu ); last = --b->live == 0; }
    if ( f.batch_item >= 0 && f.batch_item < static_cast<int>( b->items.size() ) ) b->items[f.batch_item].live = false;
    if ( last ) {
      if ( b->tokens_pending ) ctx->deferred.erase( std::remove( ctx->deferred.begin(), ctx->deferred.end(), b ), ctx->deferred.end() );
      ctx->tok.inflight.erase( std::remove( ctx->tok.inflight.begin(), ctx->tok.inflight.end(), b ), ctx->tok.inflight.end() );
      ctx->tok.batches.erase( std::remove( ctx->tok.batches.begin(), ctx->tok.batches.end(), b ), ctx->tok.batches.end() );
      if ( b->hdr_done ) { (void) hipEventSynchronize( b->hdr_done ); (void) hipEventDestroy( b->hdr_done ); }   // never forgotten while kernels still read the arena
      { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->pinned_pool.emplace_back( b->host, b->host_bytes ); }
      dev_free( ctx, b->dev, b->dev_bytes, true );        // (always through an epoch: the chunk lists of its frames are read out of it on the device)
      delete b;
    }
    f.batch = nullptr; f.summary = nullptr; f.parse_job = nullptr;
  }
  if ( f.chunk >= 0 && f.chunk < static_cast<int>( s->chunks.size() ) ) {
    Chunk & c = s->chunks[f.chunk];
    const bool is_tail = f.chunk + 1 == static_cast<int>( s->chunks.size() ) && c.host != nullptr;   // still being filled
    if ( --c.live_frames == 0 && !is_tail && c.dev ) {
      if ( c.host ) { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->pinned_pool.emplace_back( c.host, c.pinned_bytes ); c.host = nullptr; }
      dev_free( ctx, c.dev, c.dev_bytes, deferred ); c.dev = nullptr;
    }
  }
  f.host_job = nullptr; f.dev_job = nullptr;
}

uint8_t * pinned_get( aa_ctx * ctx, size_t bytes, size_t * got )
{
  {
    std::lock_guard<std::mutex> g( ctx->pool_mu );
    auto & pool = ctx->pinned_pool;
    for ( size_t i = 0; i < pool.size(); i++ )
      if ( pool[i].second >= bytes && pool[i].second <= bytes + bytes / 2 ) {
        uint8_t * p = pool[i].first; *got = pool[i].second;
        pool[i] = pool.back(); pool.pop_back();
        return p;
      }
  }
  uint8_t * p = nullptr;
  if ( hipHostMalloc( reinterpret_cast<void **>( &p ), bytes, hipHostMallocDefault ) != hipSuccess ) return nullptr;
  *got = bytes;
  { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->pinned_bytes += bytes; ctx->stats.pinned_allocs++; }
  return p;
}

// Per-frame constants of the reconstruction job record (host copy); the raster planes are bound later (bind_frame).
void fill_job( const FrameRec & rec, aa_dev_frame * job )
{
  const aa_frame_header & h = rec.hdr;
  std::memset( job, 0, sizeof *job );
  std::memcpy( job->quant, h.quant, sizeof job->quant );
  job->mbw = h.mb_width; job->mbh = h.mb_height;
  job->key_frame = h.key_frame; job->loop_filter_level = h.loop_filter_level;
  job->sharpness = h.sharpness_level; job->has_intra = h.has_intra_mb;
}

// References bookkeeping of frame `fi`, done when it is first handed to reconstruction (frames of a stream are submitted in
// order): output slot, the rasters it predicts from, then Frame::copy_to on slot ids (frame.cc:271-307).
aa_status bind_frame( aa_stream * s, int fi, aa_raster_binding * out )
{
  FrameRec & rec = s->frames[fi];
  const aa_frame_header & h = rec.hdr;
  int out_slot;
  if ( aa_status st = alloc_slot( s, &out_slot ) ) return st;
  retain( s, out_slot );   // the frame's own handle (RasterHandle returned to the caller)
  rec.out_slot = out_slot;
  out->job = const_cast<aa_dev_frame *>( rec.dev_job );
  for ( int p = 0; p < 3; p++ ) out->cur[p] = slot_plane( s, out_slot, p );
  for ( int r = 0; r < 3; r++ ) for ( int p = 0; p < 3; p++ ) out->ref[r][p] = slot_plane( s, s->cur_ref_slot[r], p );
  enum { LAST = 0, GOLDEN = 1, ALT = 2 };
  if ( h.key_frame ) { for ( int i = 0; i < 3; i++ ) set_ref( s, i, out_slot, fi ); }
  else {
    if ( h.copy_buffer_to_alternate == 1 ) set_ref( s, ALT, s->cur_ref_slot[LAST], s->cur_ref_frame[LAST] );
    else if ( h.copy_buffer_to_alternate == 2 ) set_ref( s, ALT, s->cur_ref_slot[GOLDEN], s->cur_ref_frame[GOLDEN] );
    if ( h.copy_buffer_to_golden == 1 ) set_ref( s, GOLDEN, s->cur_ref_slot[LAST], s->cur_ref_frame[LAST] );
    else if ( h.copy_buffer_to_golden == 2 ) set_ref( s, GOLDEN, s->cur_ref_slot[ALT], s->cur_ref_frame[ALT] );
    if ( h.refresh_golden ) set_ref( s, GOLDEN, out_slot, fi );
    if ( h.refresh_alternate ) set_ref( s, ALT, out_slot, fi );
    if ( h.refresh_last ) set_ref( s, LAST, out_slot, fi );
  }
  for ( int i = 0; i < 3; i++ ) rec.ref_after[i] = s->cur_ref_frame[i];
  rec.placed = true;
  if ( !rec.handle_held ) release( s, out_slot );   // the caller let go of this frame before it was decoded: only references keep its raster
  return AA_OK;
}

// Bind the rasters of the frames of a decode submission that have none yet: one small upload + one tiny kernel, in front of
// the reconstruction kernels on the compute stream.
aa_status bind_batch( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index )
{
  int need = 0;
  for ( int i = 0; i < n; i++ ) if ( !streams[i]->frames[frame_index[i]].placed ) need++;
  if ( !need ) return AA_OK;
  // pinned and mapped: the patch kernel reads the bindings over the bus.  (No copy engine on the reconstruction path: a small
  // copy queues behind whatever the engine holds, and that can be a copy ordered behind a seconds-long parse kernel.)
  JobRing::Entry * bb = nullptr;
  double waited_ms = 0;
  if ( aa_status st = ctx->bind_ring.take( size_t( need ) * sizeof( aa_raster_binding ), 512 * sizeof( aa_raster_binding ), &bb, nullptr, &waited_ms ) ) return st;
  ctx->stats.bind_wait_ms += waited_ms;
  aa_raster_binding * bindings = reinterpret_cast<aa_raster_binding *>( bb->host );
  int k = 0;
  for ( int i = 0; i < n; i++ ) {
    if ( streams[i]->frames[frame_index[i]].placed ) continue;
    if ( aa_status st = bind_frame( streams[i], frame_index[i], &bindings[k] ) ) return st;
    k++;
  }
  if ( int e = aa::launch_bind_rasters( reinterpret_cast<const aa_raster_binding *>( bb->dev ), k, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_bind_rasters" );
  return ctx->bind_ring.mark( *bb, ctx->compute );
}

// A decoded frame of this context that the caller still holds: what every call that reads a frame's raster asks first.  `who`: the
// ABI call, in front of the message; *out (may be null): the frame.
aa_status held_decoded_frame( const char * who, aa_ctx * ctx, const aa_stream * s, int fi, const FrameRec ** out )
{
  const auto no = [who]( aa_status code, const char * what ) { return fail( code, std::string( who ) + ": " + what ); };
  if ( !s || s->ctx != ctx ) return no( AA_ERR_ARGUMENT, "stream belongs to another context" );
  if ( fi < 0 || fi >= static_cast<int>( s->frames.size() ) ) return no( AA_ERR_ARGUMENT, "bad frame index" );
  const FrameRec & r = s->frames[fi];
  if ( !r.handle_held ) return no( AA_ERR_LOGIC, "frame was released" );
  if ( fi >= s->next_submit || !r.placed ) return no( AA_ERR_LOGIC, "frame not decoded yet" );
  if ( out ) *out = &r;
  return AA_OK;
}

// The persistent segment map has two homes: the host parser's (frames parsed by aa_stream_parse) and dev_segmap (frames
// parsed on the device).  Whoever parsed last owns the current copy; the other side is refreshed on demand.
aa_status segmap_to_host( aa_stream * s )
{
  if ( !s->segmap_on_device ) return AA_OK;
  for ( auto ps : s->ctx->parse_streams ) HIP_TRY( hipStreamSynchronize( ps ) );
  std::vector<uint8_t> & m = s->parser.segment_map();
  HIP_TRY( hipMemcpy( m.data(), s->dev_segmap, m.size(), hipMemcpyDeviceToHost ) );
  s->segmap_on_device = false;
  return AA_OK;
}

} // namespace
