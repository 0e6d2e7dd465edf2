// runtime.cpp, one of its pieces (ABI): rasters going out and coming in (downloads, batched delivery, references), decoder state (export /
// import, the reference's wire format), hashes and minihash.
extern "C" {
aa_status aa_stream_download( aa_stream * s, int fi, uint8_t * y, uint8_t * u, uint8_t * v )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "aa_stream_download: bad frame index" );
  const FrameRec * rp = nullptr;
  if ( aa_status st = held_decoded_frame( "aa_stream_download", s->ctx, s, fi, &rp ) ) return st;
  if ( aa_status st = set_device( s->ctx ) ) return st;
  const FrameRec & r = *rp;
  HIP_TRY( hipStreamSynchronize( s->ctx->compute ) );
  if ( aa_status st = check_watchdog( s->ctx ) ) return st;
  uint8_t * dst[3] = { y, u, v };
  for ( int p = 0; p < 3; p++ ) if ( dst[p] ) HIP_TRY( hipMemcpy( dst[p], slot_plane( s, r.out_slot, p ), s->plane_bytes[p], hipMemcpyDeviceToHost ) );
  return AA_OK;
}

/* Pinned host memory for asynchronous downloads (hipHostMalloc) */
aa_status aa_pinned_alloc( aa_ctx * ctx, size_t bytes, void ** out )
{
  if ( !ctx || !out || !bytes ) return fail( AA_ERR_ARGUMENT, "aa_pinned_alloc: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  HIP_TRY( hipHostMalloc( out, bytes, hipHostMallocDefault ) );
  return AA_OK;
}
void aa_pinned_free( void * p ) { if ( p ) (void) hipHostFree( p ); }

/* Shown frames on their way out without stalling the decoder: the copy is queued on the COPY stream behind everything the
 * compute stream holds now; the planes (pinned memory) are valid after aa_ctx_sync or aa_stream_download_wait. */
aa_status aa_stream_download_async( aa_stream * s, int fi, uint8_t * y, uint8_t * u, uint8_t * v )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "aa_stream_download_async: bad frame index" );
  const FrameRec * rp = nullptr;
  if ( aa_status st = held_decoded_frame( "aa_stream_download_async", s->ctx, s, fi, &rp ) ) return st;
  if ( aa_status st = set_device( s->ctx ) ) return st;
  const FrameRec & r = *rp;
  aa_ctx * ctx = s->ctx;
  hipEvent_t e = get_event( ctx );
  HIP_TRY( hipEventRecord( e, ctx->compute ) );
  HIP_TRY( hipStreamWaitEvent( ctx->copy, e, 0 ) );
  ctx->free_events.push_back( e );
  uint8_t * dst[3] = { y, u, v };
  // the raster may be released before the copy has run: the epoch that frees it waits for the copy stream as well
  // (the flag stays up until the event recorded behind THIS call's copies has fired: downloads are numbered, and a release on
  // another thread that finds the event of an earlier download complete does not take the flag down while a later one is still
  // between its copies and its event)
  { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->copy_reads_rasters = true; ctx->raster_download_pending = true; ++ctx->downloads_queued; }
  // Every exit -- the error exits of the HIP calls below too -- counts this download as recorded and leaves an event behind what it
  // queued on the copy stream: a download that begun and never "recorded" would keep downloads_recorded != downloads_queued for
  // the life of the context, and every raster released from then on would take the slow epoch route (ADVICE round 5).
  struct Recorded {
    aa_ctx * ctx;
    ~Recorded() {
      std::lock_guard<std::mutex> g( ctx->pool_mu );
      if ( !ctx->last_raster_download && hipEventCreateWithFlags( &ctx->last_raster_download, hipEventDisableTiming ) != hipSuccess ) { ctx->last_raster_download = nullptr; (void) hipGetLastError(); }
      if ( ctx->last_raster_download && hipEventRecord( ctx->last_raster_download, ctx->copy ) != hipSuccess ) (void) hipGetLastError();
      ++ctx->downloads_recorded;                         // (a count of finished calls: equal to downloads_queued when none is between its copies and its event)
    }
  } recorded { ctx };
  for ( int p = 0; p < 3; p++ ) if ( dst[p] ) HIP_TRY( hipMemcpyAsync( dst[p], slot_plane( s, r.out_slot, p ), s->plane_bytes[p], hipMemcpyDeviceToHost, ctx->copy ) );
  // (rasters released from now on are recycled through an epoch until this copy is through: dev_free_compute)
  return AA_OK;
}
aa_status aa_stream_download_wait( aa_stream * s )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  HIP_TRY( hipStreamSynchronize( s->ctx->copy ) );
  return check_watchdog( s->ctx );
}

/* A whole frame index of a batch on its way out (frontend/vp8decode.cc:78-93, decode-bundle.cc:92-99 deliver every shown frame): the
 * rasters of n decoded frames -- each three padded planes, contiguous in its pool piece -- are gathered by ONE kernel on the
 * compute stream into one staging piece, and ONE copy on the copy stream takes them to dst + i * stride (pinned memory).  The
 * per-plane form (aa_stream_download_async) costs 3 n copies of 0.5-2 MB: measured 16.8 GB/s over a link that does 50+. */
aa_status aa_download_batch_async( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index, uint8_t * dst, size_t stride )
{
  if ( !ctx || !streams || !frame_index || !dst || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_download_batch_async: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  size_t max_bytes = 0;
  for ( int i = 0; i < n; i++ ) {
    const aa_stream * s = streams[i];
    if ( aa_status st = held_decoded_frame( "aa_download_batch_async", ctx, s, frame_index[i], nullptr ) ) return st;
    const size_t bytes = s->plane_bytes[0] + 2 * s->plane_bytes[1];
    if ( bytes > stride ) return fail( AA_ERR_ARGUMENT, "aa_download_batch_async: stride smaller than a raster" );
    max_bytes = std::max( max_bytes, bytes );
  }
  if ( stride & 15 ) return fail( AA_ERR_ARGUMENT, "aa_download_batch_async: stride must be a multiple of 16" );
  // The entry that comes round now.  If its previous download is still on the list (more than kBindBufs queued and nobody waited for
  // it), its copy may still be writing the caller's memory, and its `copied` event -- the only handle on it -- is recorded anew below:
  // the copy is waited for HERE, before the index leaves the list, so that aa_ctx_download_wait_until never counts a running copy as
  // arrived.
  const int gi = ctx->gather_ring.next;
  hipEvent_t & copied = ctx->gather_copied[gi];
  if ( copied && std::find( ctx->downloads_in_flight.begin(), ctx->downloads_in_flight.end(), gi ) != ctx->downloads_in_flight.end() )
    HIP_TRY( hipEventSynchronize( copied ) );
  for ( auto it = ctx->downloads_in_flight.begin(); it != ctx->downloads_in_flight.end(); ) it = *it == gi ? ctx->downloads_in_flight.erase( it ) : it + 1;
  JobRing::Entry * gb = nullptr;
  if ( aa_status st = ctx->gather_ring.take( size_t( n ) * sizeof( aa_gather_job ), 512 * sizeof( aa_gather_job ), &gb ) ) return st;
  if ( !copied ) HIP_TRY( hipEventCreateWithFlags( &copied, hipEventDisableTiming ) );
  aa_gather_job * jobs = reinterpret_cast<aa_gather_job *>( gb->host );
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = streams[i];
    jobs[i].src = s->slots[s->frames[frame_index[i]].out_slot].dev;          // (Y, U, V back to back: slot_plane)
    jobs[i].bytes = s->plane_bytes[0] + 2 * s->plane_bytes[1];
  }
  const size_t total = stride * static_cast<size_t>( n );
  uint8_t * staging = nullptr;
  if ( aa_status st = dev_alloc( ctx, total, &staging ) ) return st;
  // (the piece goes back behind the copy that reads it: the epoch that frees it waits for the copy stream as well)
  struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { { std::lock_guard<std::mutex> g( c->pool_mu ); c->copy_reads_rasters = true; } dev_free( c, p, b, true ); } } back { ctx, staging, total };
  if ( int e = aa::launch_gather_rasters( reinterpret_cast<const aa_gather_job *>( gb->dev ), n, staging, stride, max_bytes, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_gather_rasters" );
  if ( aa_status st = ctx->gather_ring.mark( *gb, ctx->compute ) ) return st;
  HIP_TRY( hipStreamWaitEvent( ctx->copy, gb->done, 0 ) );
  HIP_TRY( hipMemcpyAsync( dst, staging, total, hipMemcpyDeviceToHost, ctx->copy ) );
  HIP_TRY( hipEventRecord( copied, ctx->copy ) );
  ctx->downloads_in_flight.push_back( gi );
  return AA_OK;
}
aa_status aa_ctx_download_wait( aa_ctx * ctx )
{
  if ( !ctx ) return fail( AA_ERR_ARGUMENT, "null ctx" );
  if ( aa_status st = set_device( ctx ) ) return st;
  HIP_TRY( hipStreamSynchronize( ctx->copy ) );
  ctx->downloads_in_flight.clear();
  return check_watchdog( ctx );
}
aa_status aa_ctx_download_wait_until( aa_ctx * ctx, int max_in_flight )
{
  if ( !ctx || max_in_flight < 0 ) return fail( AA_ERR_ARGUMENT, "aa_ctx_download_wait_until: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  while ( static_cast<int>( ctx->downloads_in_flight.size() ) > max_in_flight ) {
    HIP_TRY( hipEventSynchronize( ctx->gather_copied[ctx->downloads_in_flight.front()] ) );
    ctx->downloads_in_flight.pop_front();
  }
  return check_watchdog( ctx );
}

aa_status aa_stream_raster_device( aa_stream * s, int fi, void ** y, void ** u, void ** v )
{
  if ( !s || fi < 0 || fi >= static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_ARGUMENT, "bad frame index" );
  const FrameRec & r = s->frames[fi];
  if ( y ) *y = slot_plane( s, r.out_slot, 0 );
  if ( u ) *u = slot_plane( s, r.out_slot, 1 );
  if ( v ) *v = slot_plane( s, r.out_slot, 2 );
  return AA_OK;
}

/* Shown frames as RGB in the caller's device memory (VideoDisplay::draw's shader, display.cc): one k_render_rgb launch on the compute
 * stream for the lot, behind the decode of every frame it reads -- rasters are recycled in compute-stream order, so none can be
 * written under it.  Float table and job list go through a ring of pinned tables into the call's piece of the device pool. */
aa_status aa_render_rgb_async( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index, int format,
                               const aa_rgb_target * targets, const double mean[3], const double std[3], void * consumer_stream )
{
  if ( !ctx || !streams || !frame_index || !targets || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_render_rgb_async: bad argument" );
  if ( format < AA_RGB_U8_HWC3 || format > AA_RGB_F32_CHW ) return fail( AA_ERR_ARGUMENT, "aa_render_rgb_async: unknown format " + std::to_string( format ) );
  const bool is_float = format >= AA_RGB_F16_CHW, chw = format >= AA_RGB_U8_CHW;
  if ( !is_float && ( mean || std ) ) return fail( AA_ERR_ARGUMENT, "aa_render_rgb_async: mean / std apply to the float formats only" );
  if ( std ) for ( int c = 0; c < 3; c++ ) if ( std[c] == 0 ) return fail( AA_ERR_ARGUMENT, "aa_render_rgb_async: std[" + std::to_string( c ) + "] is 0" );
  if ( aa_status st = set_device( ctx ) ) return st;
  static const int kPixelBytes[6] = { 3, 4, 1, 2, 2, 4 };
  const int64_t bpp = kPixelBytes[format];
  uint64_t max_threads = 0;
  for ( int i = 0; i < n; i++ ) {
    const aa_stream * s = streams[i];
    if ( aa_status st = held_decoded_frame( "aa_render_rgb_async", ctx, s, frame_index[i], nullptr ) ) return st;
    const aa_rgb_target & t = targets[i];
    const int64_t w = s->parser.width(), h = s->parser.height();
    if ( !t.dst ) return fail( AA_ERR_ARGUMENT, "aa_render_rgb_async: null dst" );
    if ( t.row_stride < w * bpp ) return fail( AA_ERR_ARGUMENT, "aa_render_rgb_async: row stride smaller than a row" );
    if ( chw && t.plane_stride < h * t.row_stride ) return fail( AA_ERR_ARGUMENT, "aa_render_rgb_async: plane stride smaller than height * row stride" );
    max_threads = std::max<uint64_t>( max_threads, uint64_t( ( w + 15 ) / 16 ) * uint64_t( ( h + 1 ) / 2 ) );
  }
  constexpr size_t kTableBytes = 768 * sizeof( uint32_t );
  const size_t bytes = kTableBytes + size_t( n ) * sizeof( aa_rgb_job );
  JobRing::Entry * rb = nullptr;
  if ( aa_status st = ctx->rgb_ring.take( bytes, kTableBytes + 512 * sizeof( aa_rgb_job ), &rb ) ) return st;
  // float formats: out = T_c[rgb], T_c[i] = (i / 255 - mean_c) / std_c in double, rounded to float, then to half / bfloat16 (nearest even)
  uint32_t * table = reinterpret_cast<uint32_t *>( rb->host );
  if ( is_float )
    for ( int c = 0; c < 3; c++ )
      for ( int i = 0; i < 256; i++ ) {
        const float f = static_cast<float>( ( i / 255.0 - ( mean ? mean[c] : 0.0 ) ) / ( std ? std[c] : 1.0 ) );
        uint32_t bits;
        std::memcpy( &bits, &f, 4 );
        if ( format == AA_RGB_F16_CHW ) {
          const _Float16 hf = static_cast<_Float16>( f );
          uint16_t hb;
          std::memcpy( &hb, &hf, 2 );
          bits = hb;
        } else if ( format == AA_RGB_BF16_CHW ) {
          bits = ( bits & 0x7FFFFFFFu ) > 0x7F800000u ? ( bits >> 16 ) | 0x40u : ( bits + 0x7FFFu + ( ( bits >> 16 ) & 1u ) ) >> 16;
        }
        table[c * 256 + i] = bits;
      }
  aa_rgb_job * jobs = reinterpret_cast<aa_rgb_job *>( rb->host + kTableBytes );
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = streams[i];
    const int slot = s->frames[frame_index[i]].out_slot;
    aa_rgb_job & j = jobs[i];
    for ( int p = 0; p < 3; p++ ) j.plane[p] = slot_plane( s, slot, p );
    j.dst = static_cast<uint8_t *>( targets[i].dst );
    j.row_stride = targets[i].row_stride;
    j.plane_stride = chw ? targets[i].plane_stride : 0;
    j.stride_y = s->pw; j.stride_c = s->pw / 2;
    j.width = s->parser.width(); j.height = s->parser.height();
    j.groups = ( j.width + 15 ) / 16;
    j.pad = 0;
  }
  // the kernel reads table and jobs out of device memory: the call's piece of the pool, which only the compute stream touches (the
  // next owner's kernels are behind this call's)
  uint8_t * piece = nullptr;
  if ( aa_status st = dev_alloc_compute( ctx, bytes, &piece ) ) return st;
  struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { dev_free_compute( c, p, b ); } } back { ctx, piece, bytes };
  const hipStream_t consumer = static_cast<hipStream_t>( consumer_stream );
  if ( aa_status st = stream_waits_for( &ctx->rgb_consumer_ev, ctx->compute, consumer ) ) return st;
  HIP_TRY( hipMemcpyAsync( piece, rb->host, bytes, hipMemcpyHostToDevice, ctx->compute ) );
  if ( aa_status st = ctx->rgb_ring.mark( *rb, ctx->compute ) ) return st;
  if ( int e = aa::launch_render_rgb( reinterpret_cast<const aa_rgb_job *>( piece + kTableBytes ), n, format, reinterpret_cast<const uint32_t *>( piece ),
                                      static_cast<uint32_t>( max_threads ), ctx->compute ) )
    return hip_fail( static_cast<hipError_t>( e ), "k_render_rgb" );
  return stream_waits_for( &ctx->rgb_consumer_ev, consumer, ctx->compute );
}

aa_status aa_stream_references( const aa_stream * s, int * last, int * golden, int * alternate )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  int r[3] = { -1, -1, -1 };
  if ( s->next_submit > 0 ) std::memcpy( r, s->frames[s->next_submit - 1].ref_after, sizeof r );
  if ( last ) *last = r[0];
  if ( golden ) *golden = r[1];
  if ( alternate ) *alternate = r[2];
  return AA_OK;
}

aa_status aa_stream_reference_slots( const aa_stream * s, int slots[3] )
{
  if ( !s || !slots ) return fail( AA_ERR_ARGUMENT, "null argument" );
  for ( int i = 0; i < 3; i++ ) slots[i] = s->cur_ref_slot[i];
  return AA_OK;
}

aa_status aa_stream_export_raster( aa_stream * s, int fi, void * y, void * u, void * v )
{
  if ( !s || fi < 0 || fi >= static_cast<int>( s->frames.size() ) || !y || !u || !v ) return fail( AA_ERR_ARGUMENT, "aa_stream_export_raster: bad argument" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  if ( fi >= s->next_submit ) return fail( AA_ERR_LOGIC, "aa_stream_export_raster: frame not decoded yet" );
  void * dst[3] = { y, u, v };
  for ( int p = 0; p < 3; p++ )
    HIP_TRY( hipMemcpyAsync( dst[p], slot_plane( s, s->frames[fi].out_slot, p ), s->plane_bytes[p], hipMemcpyDeviceToDevice, s->ctx->compute ) );
  return AA_OK;
}
size_t aa_stream_state_size( const aa_stream * s ) { return s ? s->parser.state_size() : 0; }
aa_status aa_stream_export_state( const aa_stream * s, uint8_t * buf, size_t capacity )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  if ( aa_status st = segmap_to_host( const_cast<aa_stream *>( s ) ) ) return st;
  return export_state_common( s->parser, buf, capacity );
}
aa_status aa_stream_import_state( aa_stream * s, const uint8_t * buf, size_t size )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  if ( aa_status st = segmap_to_host( s ) ) return st;      // (also settles ownership: the imported map lives on the host side)
  return import_state_common( s->parser, buf, size );
}

/* Decoder::serialize / Decoder::deserialize (decoder.cc:54-81): [DECODER][u32 len] DecoderState References, where
 * References = [REFERENCES][u32 len][u16 display w][u16 display h][REF_LAST][u32 len] padded Y, U, V of the LAST reference
 * only (decoder.cc:177-197; golden and alternative alias it after loading, :171-175). */
aa_status aa_stream_serialize( aa_stream * s, uint8_t * buf, size_t capacity, size_t * size )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  if ( s->next_submit != static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_LOGIC, "aa_stream_serialize: parsed frames are still waiting to be decoded" );
  const int slot = s->cur_ref_slot[0];
  if ( slot < 0 ) return fail( AA_ERR_LOGIC, "aa_stream_serialize: nothing decoded or imported yet (the reference would write an uninitialised raster)" );
  if ( aa_status st = segmap_to_host( s ) ) return st;
  std::vector<uint8_t> blob;
  blob.push_back( 11 /* DECODER */ );
  blob.insert( blob.end(), 4, 0 );
  s->parser.serialize_reference( blob );
  const size_t raster = s->plane_bytes[0] + 2 * s->plane_bytes[1];
  blob.push_back( 7 /* REFERENCES */ );
  const uint32_t rlen = static_cast<uint32_t>( 4 + 5 + raster );
  for ( int i = 0; i < 4; i++ ) blob.push_back( static_cast<uint8_t>( rlen >> ( 8 * i ) ) );
  const uint16_t dims[2] = { s->parser.width(), s->parser.height() };
  for ( int k = 0; k < 2; k++ ) { blob.push_back( static_cast<uint8_t>( dims[k] ) ); blob.push_back( static_cast<uint8_t>( dims[k] >> 8 ) ); }
  blob.push_back( 8 /* REF_LAST */ );
  for ( int i = 0; i < 4; i++ ) blob.push_back( static_cast<uint8_t>( static_cast<uint32_t>( raster ) >> ( 8 * i ) ) );
  const uint32_t total = static_cast<uint32_t>( blob.size() + raster - 5 );
  for ( int i = 0; i < 4; i++ ) blob[1 + i] = static_cast<uint8_t>( total >> ( 8 * i ) );
  if ( size ) *size = blob.size() + raster;
  if ( !buf ) return AA_OK;                         // size query
  if ( capacity < blob.size() + raster ) return fail( AA_ERR_ARGUMENT, "aa_stream_serialize: buffer too small" );
  std::memcpy( buf, blob.data(), blob.size() );
  HIP_TRY( hipStreamSynchronize( s->ctx->compute ) );
  if ( aa_status st = check_watchdog( s->ctx ) ) return st;
  uint8_t * dst = buf + blob.size();
  for ( int p = 0; p < 3; p++ ) { HIP_TRY( hipMemcpy( dst, slot_plane( s, slot, p ), s->plane_bytes[p], hipMemcpyDeviceToHost ) ); dst += s->plane_bytes[p]; }
  return AA_OK;
}

static aa_status import_common( aa_stream * s, const void * const src[3], hipMemcpyKind kind );
aa_status aa_stream_deserialize( aa_stream * s, const uint8_t * buf, size_t size )
{
  if ( !s || !buf ) return fail( AA_ERR_ARGUMENT, "null argument" );
  if ( s->next_submit != static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_LOGIC, "aa_stream_deserialize: parsed frames are still waiting to be decoded" );
  if ( size < 5 || buf[0] != 11 ) return fail( AA_ERR_INVALID, "invalid decoder state: expected DECODER" );
  if ( aa_status st = segmap_to_host( s ) ) return st;
  const size_t raster = s->plane_bytes[0] + 2 * s->plane_bytes[1];
  aa::Parser trial = s->parser;                     // the stream changes only if the whole blob is good
  size_t at = 5;
  try { at += trial.deserialize_reference( buf + at, size - at ); }
  catch ( const aa::ParseError & e ) { return fail( e.code, e.message ); }
  if ( size < at + 9 + 5 + raster || buf[at] != 7 ) return fail( AA_ERR_INVALID, "invalid decoder state: expected REFERENCES" );
  const unsigned w = buf[at + 5] | ( buf[at + 6] << 8 ), h = buf[at + 7] | ( buf[at + 8] << 8 );
  at += 9;
  if ( w != s->parser.width() || h != s->parser.height() ) return fail( AA_ERR_INVALID, "invalid decoder state: reference size differs from this decoder's" );
  if ( buf[at] != 8 ) return fail( AA_ERR_INVALID, "invalid decoder state: no REF_LAST raster" );
  const size_t rl = buf[at + 1] | ( buf[at + 2] << 8 ) | ( buf[at + 3] << 16 ) | ( static_cast<size_t>( buf[at + 4] ) << 24 );
  at += 5;
  if ( rl != raster || size != at + raster ) return fail( AA_ERR_INVALID, "invalid decoder state: raster length" );
  const void * src[3] = { buf + at, buf + at + s->plane_bytes[0], buf + at + s->plane_bytes[0] + s->plane_bytes[1] };
  if ( aa_status st = import_common( s, src, hipMemcpyHostToDevice ) ) return st;
  s->parser = trial;
  return AA_OK;
}

static aa_status import_common( aa_stream * s, const void * const src[3], hipMemcpyKind kind )
{
  if ( aa_status st = set_device( s->ctx ) ) return st;
  if ( s->next_submit != static_cast<int>( s->frames.size() ) )
    return fail( AA_ERR_LOGIC, "import_reference: parsed frames are still waiting to be decoded" );
  int slot;
  if ( aa_status st = alloc_slot( s, &slot ) ) return st;
  for ( int p = 0; p < 3; p++ )
    HIP_TRY( hipMemcpyAsync( slot_plane( s, slot, p ), src[p], s->plane_bytes[p], kind, s->ctx->compute ) );
  if ( kind == hipMemcpyHostToDevice ) HIP_TRY( hipStreamSynchronize( s->ctx->compute ) );
  for ( int i = 0; i < 3; i++ ) set_ref( s, i, slot, -1 );
  return AA_OK;
}
aa_status aa_stream_import_reference( aa_stream * s, const void * y, const void * u, const void * v )
{
  if ( !s || !y || !u || !v ) return fail( AA_ERR_ARGUMENT, "null argument" );
  const void * src[3] = { y, u, v };
  return import_common( s, src, hipMemcpyDeviceToDevice );
}
aa_status aa_stream_import_reference_host( aa_stream * s, const uint8_t * y, const uint8_t * u, const uint8_t * v )
{
  if ( !s || !y || !u || !v ) return fail( AA_ERR_ARGUMENT, "null argument" );
  const void * src[3] = { y, u, v };
  return import_common( s, src, hipMemcpyHostToDevice );
}

/* ---------------- hashes (hcombine / hrange_*: runtime_types.inc) ---------------- */
namespace {
// DecoderState::hash (decoder.cc:266-281) with ProbabilityTables::hash (probability_tables.cc:36-57), Segmentation::hash
// (decoder.cc:379-394; the map is sized by the frame's PIXEL dimensions, decoder.cc:238) and FilterAdjustments::hash
// (decoder.cc:331-340 -- whose second range runs from mode_adjustments.begin() to REF_adjustments.end(), i.e. is empty: the
// mode adjustments are not hashed; kept as is).
// ... everything but the walk over the segment map.  head: dimensions and probability tables; seg: the segmentation header, the
// seed the map's chain starts from (segmentation on); filter: the adjustments (adjustments on)
struct StateHashParts { uint64_t head = 0, seg = 0, filter = 0; };
void state_hash_parts( const aa::Parser & ps, StateHashParts & out )
{
  const aa::ProbTables & t = ps.probs();
  uint64_t ph = 0;
  hrange_u8( ph, &t.coeff[0][0][0][0], 1056 ); hrange_u8( ph, t.y_mode, 4 ); hrange_u8( ph, t.uv_mode, 3 ); hrange_u8( ph, &t.mv[0][0], 38 );
  hcombine( out.head, ps.width() ); hcombine( out.head, ps.height() ); hcombine( out.head, ph );
  const aa::SegmentationState & sg = ps.segmentation();
  if ( sg.enabled ) { hcombine( out.seg, sg.absolute ? 1 : 0 ); hrange_i8( out.seg, sg.quant, 4 ); hrange_i8( out.seg, sg.lf, 4 ); }
  const aa::FilterAdjustState & fa = ps.filter_adjustments();
  if ( fa.enabled ) hrange_i8( out.filter, fa.ref, 4 );
}
uint64_t state_hash( const aa::Parser & ps )
{
  StateHashParts parts;
  state_hash_parts( ps, parts );
  uint64_t h = parts.head;
  const aa::SegmentationState & sg = ps.segmentation();
  if ( sg.enabled ) {
    uint64_t sh = parts.seg;
    const unsigned w = ps.width(), hgt = ps.height(), mbw = ps.mb_width(), mbh = ps.mb_height();
    for ( unsigned r = 0; r < hgt; r++ ) for ( unsigned c = 0; c < w; c++ ) hcombine( sh, ( r < mbh && c < mbw ) ? sg.map[size_t( r ) * mbw + c] : 3 );
    hcombine( h, sh );
  }
  if ( ps.filter_adjustments().enabled ) hcombine( h, parts.filter );
  return h;
}

// BaseRaster::raw_hash (raster.cc:52-61) of a raster slot; the recurrence is serial, so the planes come to the host
aa_status slot_hash( aa_stream * s, int slot, uint64_t * out )
{
  Slot & sl = s->slots[slot];
  if ( !sl.hash_valid ) {
    HIP_TRY( hipStreamSynchronize( s->ctx->compute ) );
    if ( aa_status st = check_watchdog( s->ctx ) ) return st;
    std::vector<uint8_t> host( s->plane_bytes[0] + 2 * s->plane_bytes[1] );
    HIP_TRY( hipMemcpy( host.data(), sl.dev, host.size(), hipMemcpyDeviceToHost ) );
    uint64_t h = 0;
    hrange_u8( h, host.data(), host.size() );
    sl.hash = h; sl.hash_valid = true;
  }
  *out = sl.hash;
  return AA_OK;
}
} // namespace

aa_status aa_parser_state_hash( const aa_parser * p, uint64_t * out )
{
  if ( !p || !out ) return fail( AA_ERR_ARGUMENT, "null argument" );
  *out = state_hash( p->impl );
  return AA_OK;
}
aa_status aa_stream_state_hash( aa_stream * s, uint64_t * out )
{
  if ( !s || !out ) return fail( AA_ERR_ARGUMENT, "null argument" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  if ( aa_status st = segmap_to_host( s ) ) return st;
  *out = state_hash( s->parser );
  return AA_OK;
}
aa_status aa_stream_raster_hash( aa_stream * s, int fi, uint64_t * out )
{
  if ( !s || !out ) return fail( AA_ERR_ARGUMENT, "aa_stream_raster_hash: bad argument" );
  const FrameRec * r = nullptr;
  if ( aa_status st = held_decoded_frame( "aa_stream_raster_hash", s->ctx, s, fi, &r ) ) return st;
  if ( aa_status st = set_device( s->ctx ) ) return st;
  return slot_hash( s, r->out_slot, out );
}
/* DecoderHash (decoder.cc:143-153,482-490): state, last, golden, alternative; everything parsed must have been submitted */
aa_status aa_stream_decoder_hash( aa_stream * s, uint64_t parts[4], uint64_t * whole )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  if ( s->next_submit != static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_LOGIC, "aa_stream_decoder_hash: parsed frames are still waiting to be decoded" );
  if ( aa_status st = segmap_to_host( s ) ) return st;
  uint64_t h[4];
  h[0] = state_hash( s->parser );
  for ( int i = 0; i < 3; i++ ) if ( aa_status st = slot_hash( s, s->cur_ref_slot[i], &h[1 + i] ) ) return st;
  if ( parts ) std::memcpy( parts, h, sizeof h );
  if ( whole ) { uint64_t w = 0; for ( int i = 0; i < 4; i++ ) hcombine( w, h[i] ); *whole = w; }
  return AA_OK;
}
aa_status aa_stream_minihash( aa_stream * s, uint32_t * out )
{
  if ( !out ) return fail( AA_ERR_ARGUMENT, "null argument" );
  uint64_t w = 0;
  if ( aa_status st = aa_stream_decoder_hash( s, nullptr, &w ) ) return st;
  *out = static_cast<uint32_t>( w );
  return AA_OK;
}

/* One frame's raster handle and records (what a dying RasterHandle gives back, raster_handle.cc:113-122) */
aa_status aa_stream_release_frame( aa_stream * s, int fi )
{
  if ( !s || fi < 0 || fi >= static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_ARGUMENT, "aa_stream_release_frame: bad frame index" );
  FrameRec & f = s->frames[fi];
  if ( f.handle_held ) { f.handle_held = false; if ( f.placed ) release( s, f.out_slot ); }
  if ( fi < s->next_submit ) release_records( s, f, true );
  std::vector<uint8_t>().swap( f.intra_diagonals );
  while ( s->first_live < static_cast<int>( s->frames.size() ) && s->frames[s->first_live].records_released && !s->frames[s->first_live].handle_held ) s->first_live++;
  return AA_OK;
}

/* References( last, golden, alternative ): Decoder( DecoderState, References ) (decoder.cc:43-46).  planes[i] = Y, U, V of
 * reference i, in HBM (is_host[i] == 0) or on the host; references whose Y pointers are equal become one raster here too. */
aa_status aa_stream_set_references( aa_stream * s, const void * const planes[3][3], const int is_host[3] )
{
  if ( !s || !planes || !is_host ) return fail( AA_ERR_ARGUMENT, "null argument" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  if ( s->next_submit != static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_LOGIC, "aa_stream_set_references: parsed frames are still waiting to be decoded" );
  int slot[3] = { -1, -1, -1 };
  bool any_host = false;
  for ( int i = 0; i < 3; i++ ) {
    for ( int p = 0; p < 3; p++ ) if ( !planes[i][p] ) return fail( AA_ERR_ARGUMENT, "aa_stream_set_references: null plane" );
    for ( int k = 0; k < i; k++ ) if ( planes[k][0] == planes[i][0] && is_host[k] == is_host[i] ) slot[i] = slot[k];
    if ( slot[i] >= 0 ) continue;
    if ( aa_status st = alloc_slot( s, &slot[i] ) ) return st;
    retain( s, slot[i] );                      // (held while the three are being set up)
    for ( int p = 0; p < 3; p++ )
      HIP_TRY( hipMemcpyAsync( slot_plane( s, slot[i], p ), planes[i][p], s->plane_bytes[p], is_host[i] ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s->ctx->compute ) );
    any_host = any_host || is_host[i];
  }
  if ( any_host ) HIP_TRY( hipStreamSynchronize( s->ctx->compute ) );       // the caller's host planes may go away
  for ( int i = 0; i < 3; i++ ) set_ref( s, i, slot[i], -1 );
  for ( int i = 0; i < 3; i++ ) { bool first = true; for ( int k = 0; k < i; k++ ) if ( slot[k] == slot[i] ) first = false; if ( first ) release( s, slot[i] ); }
  return AA_OK;
}

} // extern "C"
