// runtime.cpp, one of its pieces: the device pool (slabs, size classes, release epochs, compute-ordered recycling), events, launch timers.
namespace {

aa_status set_device( aa_ctx * ctx ) { HIP_TRY( hipSetDevice( ctx->device ) ); return AA_OK; }

constexpr size_t kSlabBytes = size_t( 256 ) << 20;

// pool_mu held.  Close the open epoch if anything was released in it (one event on the compute stream covers every launch made
// before now, hence every launch made before those releases), then hand pieces of fired epochs to the free lists.
void flush_chunk_frees( aa_ctx * ctx );     // (below)
void collect_pending( aa_ctx * ctx, bool wait_oldest )
{
  if ( ctx->open_epoch_used && ctx->binding_depth == 0 ) {
    flush_chunk_frees( ctx );           // (coefficient chunks of released frames go back behind the kernels that read them)
    hipEvent_t e = nullptr, c = nullptr;
    bool ok = hipEventCreateWithFlags( &e, hipEventDisableTiming ) == hipSuccess && hipEventRecord( e, ctx->compute ) == hipSuccess;
    // asynchronous downloads read rasters on the COPY stream: a released raster is reusable only when those copies are done too
    if ( ok && ctx->copy_reads_rasters )
      ok = hipEventCreateWithFlags( &c, hipEventDisableTiming ) == hipSuccess && hipEventRecord( c, ctx->copy ) == hipSuccess;
    if ( ok ) {
      ctx->epoch_events.push_back( { ctx->open_epoch, e, c } );
      ctx->open_epoch++; ctx->open_epoch_used = false; ctx->copy_reads_rasters = false;
    } else {
      // no event to be had: the epoch is closed by waiting for both streams instead (never left open for good)
      if ( e ) (void) hipEventDestroy( e );
      if ( c ) (void) hipEventDestroy( c );
      (void) hipGetLastError();
      if ( hipStreamSynchronize( ctx->compute ) == hipSuccess && hipStreamSynchronize( ctx->copy ) == hipSuccess ) {
        ctx->epoch_events.push_back( { ctx->open_epoch, nullptr, nullptr } );
        ctx->open_epoch++; ctx->open_epoch_used = false; ctx->copy_reads_rasters = false;
      }
    }
  }
  uint64_t fired = 0;
  while ( !ctx->epoch_events.empty() ) {
    aa_ctx::Epoch & ep = ctx->epoch_events.front();
    bool done = true;
    for ( hipEvent_t * e : { &ep.compute, &ep.copy } ) {
      if ( !*e ) continue;
      hipError_t q = hipEventQuery( *e );
      if ( q != hipSuccess && wait_oldest ) q = hipEventSynchronize( *e );
      if ( q != hipSuccess ) { done = false; break; }
      (void) hipEventDestroy( *e ); *e = nullptr;
    }
    wait_oldest = false;
    if ( !done ) { (void) hipGetLastError(); break; }
    fired = ep.id;
    ctx->epoch_events.erase( ctx->epoch_events.begin() );
  }
  if ( !fired ) return;
  size_t keep = 0;
  for ( auto & pf : ctx->pending_free ) {
    if ( pf.epoch <= fired ) ctx->dev_free[pf.bytes].push_back( pf.p );
    else ctx->pending_free[keep++] = pf;
  }
  ctx->pending_free.resize( keep );
}

// Pieces are recycled through free lists keyed by their exact size.  Streams of one frame size ask for the same few sizes --
// but a batch arena's size follows the compressed sizes of its frames, and a freed arena of a size nobody asks for again would
// sit in its list for good (measured, round 3: 130 GB of pool for 45 GB of live pieces).  So pieces that get an allocation
// of their own (more than half a slab) come in size CLASSES: a sixteenth of the next power of two (at most 6 % over).
inline size_t pool_size_class( size_t bytes )
{
  bytes = align_up( bytes );
  if ( bytes <= kSlabBytes / 2 ) return bytes;
  size_t p2 = kSlabBytes;
  while ( p2 < bytes ) p2 <<= 1;
  const size_t step = p2 / 16;
  return ( bytes + step - 1 ) / step * step;
}

// `refusable`: the piece is for frames being HANDED OVER (a batch arena): such an allocation stops a thirty-second of the limit short
// of it, so that what the caller needs to get frames OUT again -- rasters, the dense blocks of a reconstruction call -- still finds
// room; a caller that pipelines treats AA_ERR_NO_MEMORY from aa_submit_frames as "not now" and reconstructs / releases first.
aa_status dev_alloc( aa_ctx * ctx, size_t bytes, uint8_t ** out, bool refusable = false )
{
  bytes = pool_size_class( bytes );
  std::lock_guard<std::mutex> g( ctx->pool_mu );
  struct Clock { aa_ctx * c; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                 ~Clock() { c->stats.alloc_ms += std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now() - t0 ).count(); } } clock { ctx };
  int soft_waits = 0;
  for ( int attempt = 0; attempt < 3; attempt++ ) {
    auto it = ctx->dev_free.find( bytes );
    if ( it != ctx->dev_free.end() && !it->second.empty() ) { *out = it->second.back(); it->second.pop_back(); return AA_OK; }
    if ( attempt == 0 && !ctx->pending_free.empty() ) { collect_pending( ctx, false ); continue; }
    const bool big = bytes > kSlabBytes / 2;         // big pieces get their own allocation (still recycled through the free list)
    if ( !big && ctx->cur_slab && ctx->slab_used + bytes <= kSlabBytes ) { *out = ctx->cur_slab + ctx->slab_used; ctx->slab_used += bytes; return AA_OK; }
    // The pool is about to grow.  Past the soft limit, pieces that were released but may still be read by queued kernels are
    // waited for instead (they come back as the compute stream advances): the pool must not creep up to the last byte of HBM.
    const size_t grow = big ? bytes : kSlabBytes;
    if ( ctx->pool_bytes + ctx->tok.heap_mapped + grow > ctx->pool_soft_limit && !ctx->compute_free.empty() ) {
      // Past the limit: what is parked for the compute stream's own reuse (rasters and dense transients of a geometry the caller may
      // have left behind) goes back to the general lists -- through an epoch, since queued kernels may still read it.
      for ( auto & kv : ctx->compute_free ) for ( uint8_t * p : kv.second ) ctx->pending_free.push_back( { p, kv.first, ctx->open_epoch } );
      ctx->compute_free.clear(); ctx->compute_free_bytes = 0; ctx->open_epoch_used = true;
    }
    if ( ctx->pool_bytes + ctx->tok.heap_mapped + grow + ( refusable && ctx->pool_soft_limit != ~size_t( 0 ) ? ctx->pool_soft_limit / 32 : 0 ) > ctx->pool_soft_limit
         && !ctx->pending_free.empty() && soft_waits < 64 ) {
      const auto t0 = std::chrono::steady_clock::now();
      collect_pending( ctx, true );
      ctx->stats.pool_waits++;
      ctx->stats.pool_wait_ms += std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now() - t0 ).count();
      soft_waits++; attempt = 0;
      continue;
    }
    // ... and a limit that limits what the context ACCEPTS: with nothing left to wait for, the arena of a hand-over is refused
    // (repeatable: the caller reconstructs and releases frames first, or raises aa_ctx_set_memory_limit) rather than take the
    // context past what it was told it may hold.  What gets frames OUT again -- rasters, the dense blocks of a reconstruction call --
    // is never refused: it lives on the thirty-second kept back from the hand-overs, and goes past the limit only when the caller
    // holds more decoded frames at once than that covers (the pool does not re-split the free pieces of other sizes it holds).
    // (What counts is what the context HOLDS -- live pieces + mapped heap: the pool keeps freed pieces in per-size lists and does not
    // re-split them, so after a change of geometry -- or of call sizes -- it may sit on gigabytes that fit nobody; refusing by what it
    // has TAKEN would then refuse every hand-over for good.  In a run of one geometry the free lists are what the next hand-over is
    // served from, and taken ~ held.)
    const size_t keep_back = ctx->pool_soft_limit != ~size_t( 0 ) ? ctx->pool_soft_limit / 32 : 0;
    size_t idle = ctx->compute_free_bytes + ( ctx->cur_slab ? kSlabBytes - ctx->slab_used : 0 );
    for ( auto & kv : ctx->dev_free ) idle += kv.first * kv.second.size();
    const size_t held = ctx->pool_bytes > idle ? ctx->pool_bytes - idle : 0;
    if ( refusable && held + ctx->tok.heap_mapped + grow + keep_back > ctx->pool_soft_limit && ctx->pool_bytes > 0 )
      return fail( AA_ERR_NO_MEMORY, "device pool: the context's memory limit (" + std::to_string( ctx->pool_soft_limit >> 20 ) + " MiB: pool "
                                     + std::to_string( ctx->pool_bytes >> 20 ) + " + coefficient heap " + std::to_string( ctx->tok.heap_mapped >> 20 )
                                     + ") does not allow another " + std::to_string( grow >> 20 ) + " MiB: release decoded frames or raise aa_ctx_set_memory_limit" );
    hipError_t e;
    uint8_t * piece = nullptr;
    e = hipMalloc( reinterpret_cast<void **>( &piece ), grow );
    ctx->stats.slab_mallocs++;
    if ( e == hipSuccess ) {
      ctx->dev_slabs.push_back( piece ); ctx->pool_bytes += grow;
      if ( !big ) { ctx->cur_slab = piece; ctx->slab_used = bytes; }
      *out = piece;
      return AA_OK;
    }
    // out of HBM: what was released but may still be read by queued kernels comes back once they have run -- the pieces parked for
    // the compute stream's own reuse included (another context or process may hold the rest of the HBM well below this one's limit)
    (void) hipGetLastError();
    if ( !ctx->compute_free.empty() ) {
      for ( auto & kv : ctx->compute_free ) for ( uint8_t * p : kv.second ) ctx->pending_free.push_back( { p, kv.first, ctx->open_epoch } );
      ctx->compute_free.clear(); ctx->compute_free_bytes = 0; ctx->open_epoch_used = true;
    }
    if ( attempt == 2 || ctx->pending_free.empty() ) return hip_fail( e, "hipMalloc (frame store)" );
    const auto t0 = std::chrono::steady_clock::now();
    collect_pending( ctx, true );
    ctx->stats.pool_waits++;
    ctx->stats.pool_wait_ms += std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now() - t0 ).count();
  }
  return fail( AA_ERR_HIP, "device allocation failed" );
}
// `deferred`: kernels already queued may still read the piece
void dev_free( aa_ctx * ctx, uint8_t * p, size_t bytes, bool deferred = false )
{
  if ( !p ) return;
  std::lock_guard<std::mutex> g( ctx->pool_mu );
  if ( deferred ) { ctx->pending_free.push_back( { p, pool_size_class( bytes ), ctx->open_epoch } ); ctx->open_epoch_used = true; }
  else ctx->dev_free[pool_size_class( bytes )].push_back( p );
}
// A piece that only the compute stream ever touched (see aa_ctx::compute_free): reusable at once by dev_alloc_compute
void dev_free_compute( aa_ctx * ctx, uint8_t * p, size_t bytes )
{
  if ( !p ) return;
  {
    std::lock_guard<std::mutex> g( ctx->pool_mu );
    if ( ctx->raster_download_pending && ctx->last_raster_download && ctx->downloads_recorded == ctx->downloads_queued
         && hipEventQuery( ctx->last_raster_download ) == hipSuccess ) ctx->raster_download_pending = false;
    (void) hipGetLastError();
    if ( !ctx->raster_download_pending ) {
      const size_t cls = pool_size_class( bytes );
      if ( ctx->binding_depth > 0 ) ctx->compute_hold.emplace_back( p, cls );
      else { ctx->compute_free[cls].push_back( p ); ctx->compute_free_bytes += cls; }
      return;
    }
  }
  dev_free( ctx, p, bytes, true );
}
// A piece that got a device allocation of its own (more than half a slab) and that nothing queued uses any more -- the caller has waited
// for the compute stream -- goes back to the DEVICE, not to a free list: a transient of gigabytes that few later calls ask for again must
// not stay parked in a context that decodes near its memory limit.  A smaller piece takes the compute-stream route.
void dev_release_transient( aa_ctx * ctx, uint8_t * p, size_t bytes )
{
  if ( !p ) return;
  const size_t cls = pool_size_class( bytes );
  if ( cls > kSlabBytes / 2 ) {
    std::lock_guard<std::mutex> g( ctx->pool_mu );
    auto it = std::find( ctx->dev_slabs.begin(), ctx->dev_slabs.end(), p );
    if ( it != ctx->dev_slabs.end() ) {
      ctx->dev_slabs.erase( it );
      ctx->pool_bytes -= cls;
      (void) hipFree( p );
      return;
    }
  }
  dev_free_compute( ctx, p, bytes );
}
// ... and an allocation whose first use is queued on the compute stream
aa_status dev_alloc_compute( aa_ctx * ctx, size_t bytes, uint8_t ** out )
{
  {
    const size_t cls = pool_size_class( bytes );
    std::lock_guard<std::mutex> g( ctx->pool_mu );
    auto it = ctx->compute_free.find( cls );
    if ( it != ctx->compute_free.end() && !it->second.empty() ) { *out = it->second.back(); it->second.pop_back(); ctx->compute_free_bytes -= cls; return AA_OK; }
  }
  return dev_alloc( ctx, bytes, out );
}

aa_status alloc_slot( aa_stream * s, int * out )
{
  uint8_t * piece = nullptr;
  if ( aa_status st = dev_alloc_compute( s->ctx, s->slot_bytes, &piece ) ) return st;     // (written by kernels / copies queued on the compute stream)
  for ( size_t i = 0; i < s->slots.size(); i++ ) if ( !s->slots[i].dev ) { s->slots[i] = Slot(); s->slots[i].dev = piece; *out = static_cast<int>( i ); return AA_OK; }
  Slot sl; sl.dev = piece;
  *out = static_cast<int>( s->slots.size() );
  s->slots.push_back( sl );
  return AA_OK;
}
void retain( aa_stream * s, int slot ) { if ( slot >= 0 ) s->slots[slot].refs++; }
void release( aa_stream * s, int slot )
{
  if ( slot < 0 ) return;
  Slot & sl = s->slots[slot];
  if ( --sl.refs == 0 ) { if ( !sl.shared ) dev_free_compute( s->ctx, sl.dev, s->slot_bytes ); sl.dev = nullptr; sl.shared = false; }   // (kernels already queued may still read it: they are ahead of the next owner's on the compute stream)
}
void set_ref( aa_stream * s, int which, int slot, int frame )
{
  retain( s, slot ); release( s, s->cur_ref_slot[which] );
  s->cur_ref_slot[which] = slot; s->cur_ref_frame[which] = frame;
}

aa_status reserve( aa_stream * s, size_t bytes, Chunk ** out )
{
  if ( s->chunks.empty() || !s->chunks.back().dev || s->chunks.back().used + bytes > s->chunks.back().capacity ) {
    if ( !s->chunks.empty() && s->chunks.back().dev && s->chunks.back().live_frames == 0 ) {   // every frame of the old tail is gone already
      Chunk & t = s->chunks.back();
      if ( t.host ) { std::lock_guard<std::mutex> g( s->ctx->pool_mu ); s->ctx->pinned_pool.emplace_back( t.host, t.pinned_bytes ); t.host = nullptr; }
      dev_free( s->ctx, t.dev, t.dev_bytes, true ); t.dev = nullptr;
    }
    Chunk c;
    c.capacity = std::max( kChunkBytes, align_up( bytes ) );
    {
      std::lock_guard<std::mutex> g( s->ctx->pool_mu );
      auto & pool = s->ctx->pinned_pool;
      for ( size_t i = 0; i < pool.size(); i++ ) if ( pool[i].second == c.capacity ) { c.host = pool[i].first; pool[i] = pool.back(); pool.pop_back(); break; }
    }
    if ( !c.host ) { HIP_TRY( hipHostMalloc( reinterpret_cast<void **>( &c.host ), c.capacity, hipHostMallocDefault ) ); std::lock_guard<std::mutex> g( s->ctx->pool_mu ); s->ctx->pinned_bytes += c.capacity; }
    c.pinned_bytes = c.dev_bytes = c.capacity;
    if ( aa_status st = dev_alloc( s->ctx, c.capacity, &c.dev ) ) { std::lock_guard<std::mutex> g( s->ctx->pool_mu ); s->ctx->pinned_pool.emplace_back( c.host, c.pinned_bytes ); return st; }
    s->chunks.push_back( c );
  }
  *out = &s->chunks.back();
  return AA_OK;
}

hipEvent_t get_event( aa_ctx * ctx )
{
  if ( !ctx->free_events.empty() ) { hipEvent_t e = ctx->free_events.back(); ctx->free_events.pop_back(); return e; }
  hipEvent_t e = nullptr; (void) hipEventCreate( &e ); return e;
}
// `waiter` takes up what is queued on it from now on only when everything `ahead` holds now has run.  A null stream: no caller's
// stream to order against (aa_render_rgb_async, quality_of_planes).  *ev: the owner's event, made at the first use; one serves
// every call of the owner's, since a queued wait keeps the record it was queued behind.
aa_status stream_waits_for( hipEvent_t * ev, hipStream_t waiter, hipStream_t ahead )
{
  if ( !waiter || !ahead ) return AA_OK;
  if ( !*ev ) HIP_TRY( hipEventCreateWithFlags( ev, hipEventDisableTiming ) );
  HIP_TRY( hipEventRecord( *ev, ahead ) );
  HIP_TRY( hipStreamWaitEvent( waiter, *ev, 0 ) );
  return AA_OK;
}
void drain_profile( aa_ctx * ctx )
{
  for ( auto & t : ctx->pending ) {
    float ms = 0;
    if ( hipEventSynchronize( t.b ) == hipSuccess && hipEventElapsedTime( &ms, t.a, t.b ) == hipSuccess ) {
      if ( t.kind == 0 ) { ctx->stats.recon_inter_ms += ms; ctx->stats.recon_inter_launches++; }
      else if ( t.kind == 1 ) { ctx->stats.recon_intra_ms += ms; ctx->stats.recon_intra_launches++; }
      else if ( t.kind == 2 ) { ctx->stats.loopfilter_ms += ms; ctx->stats.loopfilter_launches++; }
      else if ( t.kind == 3 ) { ctx->stats.parse_headers_ms += ms; ctx->stats.parse_launches++; }
      else if ( t.kind == 4 ) ctx->stats.parse_tokens_ms += ms;
      else if ( t.kind == 6 ) { /* (the expansion pass: gone since round 6) */ }
      else { ctx->stats.recon_split_ms += ms; ctx->stats.recon_split_launches++; }
    }
    ctx->free_events.push_back( t.a ); ctx->free_events.push_back( t.b );
  }
  ctx->pending.clear();
}

aa_status ensure_ws( aa_ctx * ctx, aa_sync_ws ** ws, size_t * have, int max_mbh )
{
  const size_t need = sizeof( aa_sync_ws ) + sizeof( int ) * size_t( AA_MAX_BATCH ) * max_mbh;
  if ( need <= *have ) return AA_OK;
  HIP_TRY( hipStreamSynchronize( ctx->compute ) );
  int err = 0;
  if ( *ws ) { (void) hipMemcpy( &err, &( *ws )->error, sizeof err, hipMemcpyDeviceToHost ); (void) hipFree( *ws ); }
  *ws = nullptr; *have = 0;
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( ws ), need ) );
  // (hipMemset of device memory is not ordered against the context's NON-BLOCKING streams: everything that prepares memory a
  // kernel on one of them will use is either queued on that stream or followed by a device-wide wait)
  HIP_TRY( hipMemsetAsync( *ws, 0, need, ctx->compute ) );
  HIP_TRY( hipStreamSynchronize( ctx->compute ) );
  if ( err ) HIP_TRY( hipMemcpy( &( *ws )->error, &err, sizeof err, hipMemcpyHostToDevice ) );   // the error word is sticky
  *have = need;
  return AA_OK;
}
aa_status zero_ws( aa_ctx * ctx, aa_sync_ws * ws, int frames, int max_mbh )
{
  HIP_TRY( hipMemsetAsync( reinterpret_cast<uint8_t *>( ws ) + AA_SYNC_WS_ZERO_FROM, 0,
                           sizeof( aa_sync_ws ) - AA_SYNC_WS_ZERO_FROM + sizeof( int ) * size_t( frames ) * max_mbh, ctx->compute ) );
  return AA_OK;
}
struct LaunchTimer {     // events on the stream the kernel is launched on
  aa_ctx * ctx; int kind; hipEvent_t a = nullptr; hipStream_t st;
  LaunchTimer( aa_ctx * c, int k, hipStream_t on = nullptr ) : ctx( c ), kind( k ), st( on ? on : c->compute ) { if ( ctx->profile ) { a = get_event( ctx ); (void) hipEventRecord( a, st ); } }
  ~LaunchTimer() { if ( ctx->profile ) { hipEvent_t b = get_event( ctx ); (void) hipEventRecord( b, st ); ctx->pending.push_back( { a, b, kind } ); if ( ctx->pending.size() >= 8192 ) drain_profile( ctx ); } }
};

} // namespace
