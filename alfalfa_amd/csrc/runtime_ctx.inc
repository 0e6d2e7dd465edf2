// runtime.cpp, one of its pieces (ABI): errors, the host parser's entry points, contexts (create / destroy / info / limits / switches), streams.

extern "C" {

const char * aa_last_error( void ) { return g_last_error.c_str(); }
int aa_host_cpus( void ) { return effective_cpus(); }
int aa_runtime_prepare( void )
{
  // (overwrite = 0: a value the host program or its user chose stands)
  const bool was_set = std::getenv( "GPU_MAX_HW_QUEUES" ) != nullptr;
  setenv( "GPU_MAX_HW_QUEUES", "16", 0 );
  return was_set ? 1 : 0;
}
int aa_abi_version( void ) { return AA_ABI_VERSION; }
int aa_device_count( void ) { int n = 0; if ( hipGetDeviceCount( &n ) != hipSuccess ) return 0; return n; }

void aa_raster_geometry( uint16_t width, uint16_t height, uint32_t * pw, uint32_t * ph )
{
  if ( pw ) *pw = 16u * ( ( width + 15u ) / 16u );
  if ( ph ) *ph = 16u * ( ( height + 15u ) / 16u );
}

/* ---------------- parser ---------------- */
aa_status aa_parser_create( uint16_t width, uint16_t height, aa_parser ** out )
{
  if ( !out || !width || !height ) return fail( AA_ERR_ARGUMENT, "aa_parser_create: bad argument" );
  *out = new ( std::nothrow ) aa_parser( width, height );
  return *out ? AA_OK : fail( AA_ERR_ARGUMENT, "out of memory" );
}
void aa_parser_destroy( aa_parser * p ) { delete p; }

aa_status aa_parser_parse( aa_parser * p, const uint8_t * data, size_t size, aa_frame_header * hdr, aa_mb_info * mb, int16_t * coeff )
{
  if ( !p || !data || !hdr || !mb || !coeff ) return fail( AA_ERR_ARGUMENT, "aa_parser_parse: null argument" );
  try { p->impl.parse( data, size, *hdr, mb, coeff ); }
  catch ( const aa::ParseError & e ) { return fail( e.code, e.message ); }
  return AA_OK;
}
aa_status aa_parse_frame_tag( const uint8_t * data, size_t size, uint16_t width, uint16_t height, int accept_partial,
                              int * key_frame, int * show_frame, int * experimental, int * corruption_level )
{
  if ( !data && size ) return fail( AA_ERR_ARGUMENT, "aa_parse_frame_tag: null data" );
  try {
    const aa::FrameTag t = aa::parse_frame_tag( data, size, width, height, accept_partial != 0 );
    if ( key_frame ) *key_frame = t.key; if ( show_frame ) *show_frame = t.show;
    if ( experimental ) *experimental = t.experimental; if ( corruption_level ) *corruption_level = t.corruption;
  } catch ( const aa::ParseError & e ) { return fail( e.code, e.message ); }
  return AA_OK;
}
aa_status aa_parser_set_error_concealment( aa_parser * p, int on )
{
  if ( !p ) return fail( AA_ERR_ARGUMENT, "null parser" );
  p->impl.set_error_concealment( on != 0 );
  return AA_OK;
}
static void export_probs( const aa::Parser & ps, uint8_t * out )
{
  const aa::ProbTables & t = ps.probs();
  std::memcpy( out, t.coeff, 1056 ); std::memcpy( out + 1056, t.y_mode, 4 );
  std::memcpy( out + 1060, t.uv_mode, 3 ); std::memcpy( out + 1063, t.mv, 38 );
}
aa_status aa_parser_get_probs( const aa_parser * p, uint8_t probs[1101] )
{
  if ( !p || !probs ) return fail( AA_ERR_ARGUMENT, "null argument" );
  export_probs( p->impl, probs ); return AA_OK;
}
aa_status aa_parser_get_segmentation( const aa_parser * p, int * enabled, int * absolute, int8_t quant[4], int8_t lf[4], uint8_t * map )
{
  if ( !p ) return fail( AA_ERR_ARGUMENT, "null argument" );
  const aa::SegmentationState & s = p->impl.segmentation();
  if ( enabled ) *enabled = s.enabled;
  if ( absolute ) *absolute = s.absolute;
  if ( quant ) std::memcpy( quant, s.quant, 4 );
  if ( lf ) std::memcpy( lf, s.lf, 4 );
  if ( map ) std::memcpy( map, s.map.data(), s.map.size() );
  return AA_OK;
}
aa_status aa_parser_get_filter_adjustments( const aa_parser * p, int * enabled, int8_t ref[4], int8_t mode[4] )
{
  if ( !p ) return fail( AA_ERR_ARGUMENT, "null argument" );
  const aa::FilterAdjustState & f = p->impl.filter_adjustments();
  if ( enabled ) *enabled = f.enabled;
  if ( ref ) std::memcpy( ref, f.ref, 4 );
  if ( mode ) std::memcpy( mode, f.mode, 4 );
  return AA_OK;
}

static aa_status export_state_common( const aa::Parser & ps, uint8_t * buf, size_t capacity )
{
  if ( !buf || capacity < ps.state_size() ) return fail( AA_ERR_ARGUMENT, "export_state: buffer too small" );
  ps.export_state( buf ); return AA_OK;
}
static aa_status import_state_common( aa::Parser & ps, const uint8_t * buf, size_t size )
{
  if ( !buf ) return fail( AA_ERR_ARGUMENT, "import_state: null buffer" );
  try { ps.import_state( buf, size ); } catch ( const aa::ParseError & e ) { return fail( e.code, e.message ); }
  return AA_OK;
}
size_t aa_parser_state_size( const aa_parser * p ) { return p ? p->impl.state_size() : 0; }
aa_status aa_parser_export_state( const aa_parser * p, uint8_t * buf, size_t capacity )
{ return p ? export_state_common( p->impl, buf, capacity ) : fail( AA_ERR_ARGUMENT, "null parser" ); }
aa_status aa_parser_import_state( aa_parser * p, const uint8_t * buf, size_t size )
{ return p ? import_state_common( p->impl, buf, size ) : fail( AA_ERR_ARGUMENT, "null parser" ); }

/* DecoderState in the reference's wire format (DecoderState::serialize, decoder.cc:283-313) */
static aa_status serialize_out( const std::vector<uint8_t> & blob, uint8_t * buf, size_t capacity, size_t * size )
{
  if ( size ) *size = blob.size();
  if ( !buf ) return AA_OK;                         // size query
  if ( capacity < blob.size() ) return fail( AA_ERR_ARGUMENT, "serialize: buffer too small" );
  std::memcpy( buf, blob.data(), blob.size() );
  return AA_OK;
}
aa_status aa_parser_serialize_state( const aa_parser * p, uint8_t * buf, size_t capacity, size_t * size )
{
  if ( !p ) return fail( AA_ERR_ARGUMENT, "null parser" );
  std::vector<uint8_t> blob;
  p->impl.serialize_reference( blob );
  return serialize_out( blob, buf, capacity, size );
}
aa_status aa_parser_deserialize_state( aa_parser * p, const uint8_t * buf, size_t size )
{
  if ( !p || !buf ) return fail( AA_ERR_ARGUMENT, "null argument" );
  aa::Parser trial = p->impl;                        // the parser changes only if the whole blob is good
  try { if ( trial.deserialize_reference( buf, size ) != size ) return fail( AA_ERR_INVALID, "invalid decoder state: trailing bytes" ); }
  catch ( const aa::ParseError & e ) { return fail( e.code, e.message ); }
  p->impl = trial;
  return AA_OK;
}

/* ---------------- context ---------------- */
aa_status aa_ctx_create( int device, aa_ctx ** out )
{
  if ( !out ) return fail( AA_ERR_ARGUMENT, "aa_ctx_create: null out" );
  int n = 0;
  hipError_t e = hipGetDeviceCount( &n );
  if ( e != hipSuccess || n == 0 )
    return fail( AA_ERR_NO_DEVICE, "no HIP device visible: the decode path has no CPU fallback" );
  if ( device < 0 || device >= n ) return fail( AA_ERR_ARGUMENT, "device index out of range" );
  std::unique_ptr<aa_ctx> ctx( new aa_ctx );
  ctx->device = device;
  HIP_TRY( hipSetDevice( device ) );
  {
    // reconstruction is short and latency-critical, the entropy decode long and patient: the compute stream gets the
    // highest priority the device offers, the parse streams the lowest
    int lo = 0, hi = 0;
    HIP_TRY( hipDeviceGetStreamPriorityRange( &lo, &hi ) );
    ctx->prio_low = lo;
    HIP_TRY( hipStreamCreateWithPriority( &ctx->compute, hipStreamNonBlocking, hi ) );
  }
  HIP_TRY( hipStreamCreateWithFlags( &ctx->copy, hipStreamNonBlocking ) );
  HIP_TRY( hipEventCreateWithFlags( &ctx->upload_done, hipEventDisableTiming ) );
  {
    size_t free_b = 0, total_b = 0;
    if ( hipMemGetInfo( &free_b, &total_b ) == hipSuccess && free_b ) ctx->pool_soft_limit = free_b / 8 * 7;
    (void) hipGetLastError();
  }
  if ( const char * e = getenv( "ALFALFA_AMD_PARSE_STREAMS" ) ) ctx->n_parse_streams = std::max( 1, std::min( aa_ctx::kMaxParseStreams, atoi( e ) ) );
  ctx->parse_streams.assign( ctx->n_parse_streams, nullptr );
  ctx->parse_idle.assign( ctx->n_parse_streams, nullptr );
  for ( auto & ps : ctx->parse_streams ) HIP_TRY( hipStreamCreateWithPriority( &ps, hipStreamNonBlocking, ctx->prio_low ) );
  for ( auto & e : ctx->parse_idle ) HIP_TRY( hipEventCreateWithFlags( &e, hipEventDisableTiming ) );
  if ( const char * e = std::getenv( "ALFALFA_AMD_SCHEDULE" ) ) ctx->schedule = std::string( e ) == "diagonal" ? 1 : 0;
  if ( const char * e = std::getenv( "ALFALFA_AMD_PACKED" ) ) ctx->tok.packed = atoi( e ) != 0;
  if ( const char * e = std::getenv( "ALFALFA_AMD_LANE_PER_PARTITION" ) ) ctx->tok.lane_per_partition = atoi( e ) != 0;
  if ( const char * e = std::getenv( "ALFALFA_AMD_REENC_SLOTS" ) ) ctx->reenc_slots = std::max( 1, std::min( 16, atoi( e ) ) );
  if ( const char * e = std::getenv( "ALFALFA_AMD_HOST_SHARE_MS" ) ) ctx->host_share_ms = std::max( 0.0, atof( e ) );
  // The row-pipelined kernels keep every unit on one XCD (per-XCD ticket queues indexed by the hardware XCC_ID): find
  // out which XCC ids workgroups of this device really land on.  They must be 0..n-1, each reached by a modest grid.
  {
    int * d = nullptr; int h[AA_MAX_XCD] = {};
    HIP_TRY( hipMalloc( reinterpret_cast<void **>( &d ), sizeof h ) );
    // (on the probe's own stream: a plain hipMemset is not ordered against a non-blocking stream, and under load -- other contexts'
    // worker grids resident -- it was seen to land AFTER the probe kernel: "XCD probe kernel did not run")
    HIP_TRY( hipMemsetAsync( d, 0, sizeof h, ctx->compute ) );
    const int e2 = aa::launch_probe_xcds( d, 2048, ctx->compute );
    if ( e2 ) { (void) hipFree( d ); return hip_fail( static_cast<hipError_t>( e2 ), "k_probe_xcds" ); }
    HIP_TRY( hipStreamSynchronize( ctx->compute ) );
    HIP_TRY( hipMemcpy( h, d, sizeof h, hipMemcpyDeviceToHost ) );
    (void) hipFree( d );
    int n_xcd = 0;
    while ( n_xcd < AA_MAX_XCD && h[n_xcd] > 0 ) n_xcd++;
    for ( int x = n_xcd; x < AA_MAX_XCD; x++ ) if ( h[x] ) return fail( AA_ERR_HIP, "unexpected XCC id layout on this device (ids are not 0..n-1)" );
    if ( n_xcd == 0 ) return fail( AA_ERR_HIP, "XCD probe kernel did not run" );
    for ( int x = 0; x < n_xcd; x++ ) ctx->xcd_share[x] = h[x];
    ctx->n_xcd = n_xcd;
    // The row-pipelined schedule wants every XCD to get its share of a launch's workgroups (the observed round-robin).  If this
    // device spreads them unevenly (CU masks, partition modes), fall back to the schedule whose ordering is kernel boundaries.
    for ( int x = 0; x < n_xcd; x++ ) if ( h[x] * n_xcd * 2 < 2048 ) ctx->schedule = 1;
  }
  *out = ctx.release();
  return AA_OK;
}
static void ctx_free( aa_ctx * ctx );
void aa_ctx_destroy( aa_ctx * ctx )
{
  if ( !ctx ) return;
  (void) hipSetDevice( ctx->device );
  hash_drain( ctx );                    // (outstanding hash calls write the caller's arrays at their wait: not after the handle is gone)
  if ( --ctx->refs == 0 ) ctx_free( ctx );
}
static void ctx_free( aa_ctx * ctx )
{
  (void) hipSetDevice( ctx->device );
  (void) tok_quiesce( ctx );
  host_lanes_stop( ctx );
  (void) hipStreamSynchronize( ctx->compute ); (void) hipStreamSynchronize( ctx->copy );
  for ( auto ps : ctx->parse_streams ) if ( ps ) { (void) hipStreamSynchronize( ps ); (void) hipStreamDestroy( ps ); }
  for ( auto e : ctx->parse_idle ) if ( e ) (void) hipEventDestroy( e );
  for ( auto & ee : ctx->epoch_events ) { if ( ee.compute ) (void) hipEventDestroy( ee.compute ); if ( ee.copy ) (void) hipEventDestroy( ee.copy ); }
  if ( ctx->last_seg_batch ) (void) hipEventDestroy( ctx->last_seg_batch );
  drain_profile( ctx );
  for ( auto e : ctx->free_events ) (void) hipEventDestroy( e );
  (void) hipEventDestroy( ctx->upload_done );
  if ( ctx->last_raster_download ) (void) hipEventDestroy( ctx->last_raster_download );
  hash_free( ctx );
  for ( JobRing * r : { &ctx->bind_ring, &ctx->gather_ring, &ctx->rgb_ring, &ctx->quality_ring, &ctx->rebase_ring, &ctx->lf_ring } ) r->destroy();
  for ( hipEvent_t e : ctx->gather_copied ) if ( e ) (void) hipEventDestroy( e );
  for ( hipEvent_t e : { ctx->rgb_consumer_ev, ctx->quality_consumer_ev } ) if ( e ) (void) hipEventDestroy( e );
  if ( ctx->ws ) (void) hipFree( ctx->ws );
  if ( ctx->boundary ) (void) hipFree( ctx->boundary );
  tok_free( ctx );
  for ( auto & pc : ctx->pinned_pool ) (void) hipHostFree( pc.first );
  for ( uint8_t * slab : ctx->dev_slabs ) (void) hipFree( slab );
  (void) hipStreamDestroy( ctx->compute ); (void) hipStreamDestroy( ctx->copy );
  delete ctx;
}
static aa_status check_watchdog( aa_ctx * ctx )
{
  if ( !ctx->ws ) return AA_OK;
  int err = 0;
  HIP_TRY( hipMemcpy( &err, &ctx->ws->error, sizeof err, hipMemcpyDeviceToHost ) );
  if ( err == 3 ) return fail( AA_ERR_HIP, "row-pipelined kernel: a workgroup ran on an XCD outside the probed set (output is not valid)" );
  if ( err == 5 ) {
    int hdr[4] = {};
    (void) hipMemcpy( hdr, ctx->ws, sizeof hdr, hipMemcpyDeviceToHost );
    return fail( AA_ERR_HIP, "row-pipelined kernel: XCD " + std::to_string( hdr[1] ) + " handed out " + std::to_string( hdr[2] ) + " of its " + std::to_string( hdr[3] )
                               + " macroblock rows: no workgroup of the launch ran there (output is not valid); use the diagonal schedule on this device" );
  }
  if ( err == 4 ) {
    int hdr[4] = {};
    (void) hipMemcpy( hdr, ctx->ws, sizeof hdr, hipMemcpyDeviceToHost );
    return fail( AA_ERR_HIP, "row-pipelined kernel: a wave of unit " + std::to_string( hdr[1] ) + " row " + std::to_string( hdr[2] ) + " moved from XCD "
                               + std::to_string( hdr[3] >> 16 ) + " to XCD " + std::to_string( hdr[3] & 0xFFFF ) + " (context save/restore under queue oversubscription?): "
                               "the in-launch hand-off is only coherent inside one XCD (output is not valid)" );
  }
  if ( err ) {
    int hdr[4 + AA_SYNC_WS_DUMP + AA_MAX_XCD] = {};
    (void) hipMemcpy( hdr, ctx->ws, sizeof hdr, hipMemcpyDeviceToHost );
    std::string tickets, rows;
    for ( int x = 0; x < ctx->n_xcd; x++ ) tickets += ( x ? "," : "" ) + std::to_string( hdr[4 + AA_SYNC_WS_DUMP + x] );
    const int * dump = hdr + 4;
    for ( int r = 0; r < std::min( 128, dump[130] ); r++ ) rows += ( r ? "," : "" ) + std::to_string( dump[r] );
    return fail( AA_ERR_HIP, std::string( "row-pipelined kernel " ) + ( err == 1 ? "k_recon_intra4" : "k_loopfilter_rows4" )
                               + ": a bounded wait for the macroblock row above expired (output is not valid); first at unit " + std::to_string( hdr[1] )
                               + " row " + std::to_string( hdr[2] ) + ", needed " + std::to_string( hdr[3] >> 16 ) + " saw " + std::to_string( hdr[3] & 0xFFFF )
                               + " after " + std::to_string( dump[128] ) + " polls in " + std::to_string( dump[129] ) + " ms; columns done per row of that unit when it gave up: " + rows
                               + "; tickets handed out per XCD (last launch): " + tickets );
  }
  return AA_OK;
}
aa_status aa_ctx_sync( aa_ctx * ctx )
{
  if ( !ctx ) return fail( AA_ERR_ARGUMENT, "null ctx" );
  if ( aa_status st = set_device( ctx ) ) return st;
  HIP_TRY( hipStreamSynchronize( ctx->copy ) );
  for ( auto ps : ctx->parse_streams ) HIP_TRY( hipStreamSynchronize( ps ) );
  if ( aa_status st = tok_quiesce( ctx ) ) return st;       // every frame handed to the token workers is parsed
  { std::lock_guard<std::mutex> g( ctx->pool_mu ); flush_chunk_frees( ctx ); }     // coefficient chunks of released frames are back in the pool
  HIP_TRY( hipStreamSynchronize( ctx->compute ) );
  return check_watchdog( ctx );
}
aa_status aa_ctx_memory( aa_ctx * ctx, size_t * free_bytes, size_t * total_bytes )
{
  if ( !ctx ) return fail( AA_ERR_ARGUMENT, "null ctx" );
  if ( aa_status st = set_device( ctx ) ) return st;
  size_t f = 0, t = 0;
  HIP_TRY( hipMemGetInfo( &f, &t ) );
  if ( free_bytes ) *free_bytes = f;
  if ( total_bytes ) *total_bytes = t;
  return AA_OK;
}
aa_status aa_ctx_set_memory_limit( aa_ctx * ctx, size_t bytes )
{
  if ( !ctx || !bytes ) return fail( AA_ERR_ARGUMENT, "aa_ctx_set_memory_limit: bad argument" );
  std::lock_guard<std::mutex> g( ctx->pool_mu );
  ctx->pool_soft_limit = bytes;
  if ( !ctx->tok.ready ) ctx->tok.heap_limit = 0;      // (the heap's virtual size follows the limit when it is set up)
  return AA_OK;
}
aa_status aa_ctx_get_info( aa_ctx * ctx, aa_ctx_info * out )
{
  if ( !ctx || !out ) return fail( AA_ERR_ARGUMENT, "null argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  std::memset( out, 0, sizeof *out );
  auto & T = ctx->tok;
  {
    std::lock_guard<std::mutex> g( ctx->pool_mu );
    collect_pending( ctx, false );        // (pieces whose release epoch has fired are free, not pending: a caller that plans by these figures should see that)
    out->memory_limit_bytes = ctx->pool_soft_limit; out->pool_bytes = ctx->pool_bytes; out->pinned_host_bytes = ctx->pinned_bytes;
    for ( auto & kv : ctx->dev_free ) out->pool_free_bytes += kv.first * kv.second.size();
    for ( auto & pf : ctx->pending_free ) out->pool_pending_bytes += pf.bytes;
    if ( ctx->cur_slab ) out->pool_free_bytes += kSlabBytes - ctx->slab_used;
    out->pool_free_bytes += ctx->compute_free_bytes;
    for ( auto & h : ctx->compute_hold ) out->pool_pending_bytes += h.second;
  }
  out->heap_mapped_bytes = T.heap_mapped; out->heap_limit_bytes = T.heap_va;
  out->heap_used_bytes = static_cast<uint64_t>( std::max<int64_t>( 0, T.chunks_committed ) ) * kChunkBytesHeap;
  out->heap_is_virtual = T.vmm ? 1u : 0u;
  out->packed_coefficients = T.packed ? 1u : 0u;
  out->lane_per_partition = T.lane_per_partition ? 1u : 0u;
  out->token_lanes_per_workgroup = static_cast<uint32_t>( T.lanes ); out->token_workgroups_capacity = static_cast<uint32_t>( T.cap_wgs );
  out->token_lane_lds_bytes = T.lane_bytes; out->token_workgroup_lds_bytes = T.lds;
  out->compute_units = static_cast<uint32_t>( T.n_cus );
  out->host_share_ms = static_cast<uint32_t>( ctx->host_share_ms + 0.5 );
  out->host_rate_kb_per_ms = ctx->host_lanes.parse_us.load() ? static_cast<uint32_t>( host_lanes_rate( ctx ) / 1e3 + 0.5 ) : 0u;
  out->stream_concurrency = ctx->stream_concurrency; out->streams_needed = ctx->streams_needed;
  out->host_waited_parse_ms = static_cast<uint32_t>( ctx->stats.parse_wait_ms ); out->host_waited_compute_ms = static_cast<uint32_t>( ctx->stats.bind_wait_ms );
  // (asked once: the attribute query goes to the driver and was seen to take ~100 ms beside a busy GPU -- three looks at the books per
  // step of a pipelining caller were 300 ms of its step)
  if ( !ctx->clock_mhz ) { int khz = 0; if ( hipDeviceGetAttribute( &khz, hipDeviceAttributeClockRate, ctx->device ) == hipSuccess ) ctx->clock_mhz = static_cast<uint32_t>( khz / 1000 ); else (void) hipGetLastError(); }
  out->clock_mhz = ctx->clock_mhz;
  if ( T.ready ) {
    if ( aa_status st = tok_peek_mirror( ctx ) ) return st;
    out->heap_free_chunks = T.mirror_host->pool_avail; out->lanes_starved = T.mirror_host->pool_starving;
    for ( int k = 0; k < 8; k++ ) out->token_profile[k] = T.mirror_host->prof[k];
    uint32_t alive = 0;
    for ( int g = 0; g < aa_ctx::Tok::kSlots; g++ ) alive += T.slot[g].launched - T.mirror_host->exited[g];
    out->token_workgroups_alive = alive;
    const int32_t waiting = static_cast<int32_t>( static_cast<uint32_t>( T.jobs_enqueued ) - T.mirror_host->q_head );
    out->jobs_waiting = waiting > 0 ? static_cast<uint32_t>( waiting ) : 0u;
  }
  return AA_OK;
}
aa_status aa_ctx_set_lane_per_partition( aa_ctx * ctx, int on )
{
  if ( !ctx ) return fail( AA_ERR_ARGUMENT, "null context" );
  if ( ctx->tok.ready && ctx->tok.lane_per_partition != ( on != 0 ) ) return fail( AA_ERR_LOGIC, "aa_ctx_set_lane_per_partition: frames have been submitted to this context already" );
  ctx->tok.lane_per_partition = on != 0;
  return AA_OK;
}
aa_status aa_ctx_set_host_share_ms( aa_ctx * ctx, double ms )
{
  if ( !ctx || !( ms >= 0 ) ) return fail( AA_ERR_ARGUMENT, "aa_ctx_set_host_share_ms: bad argument" );
  ctx->host_share_ms = ms;
  return AA_OK;
}
aa_status aa_ctx_set_packed_coefficients( aa_ctx * ctx, int on )
{
  if ( !ctx ) return fail( AA_ERR_ARGUMENT, "null context" );
  if ( ctx->tok.ready && ctx->tok.packed != ( on != 0 ) ) return fail( AA_ERR_LOGIC, "aa_ctx_set_packed_coefficients: frames have been submitted to this context already" );
  ctx->tok.packed = on != 0;
  return AA_OK;
}
/* The sticky error word of the row-pipelined kernels (a bounded wait expired, a wave found itself on another XCD, a queue
 * was not drained) makes every later row-pipelined launch give up early.  Once it has been reported, this clears it. */
aa_status aa_ctx_clear_error( aa_ctx * ctx )
{
  if ( !ctx ) return fail( AA_ERR_ARGUMENT, "null ctx" );
  if ( aa_status st = set_device( ctx ) ) return st;
  HIP_TRY( hipStreamSynchronize( ctx->compute ) );
  if ( ctx->ws ) { HIP_TRY( hipMemsetAsync( ctx->ws, 0, AA_SYNC_WS_ZERO_FROM, ctx->compute ) ); HIP_TRY( hipStreamSynchronize( ctx->compute ) ); }
  return AA_OK;
}
aa_status aa_ctx_set_schedule( aa_ctx * ctx, int schedule )
{
  if ( !ctx || ( schedule != AA_SCHEDULE_ROWS && schedule != AA_SCHEDULE_DIAGONAL ) ) return fail( AA_ERR_ARGUMENT, "aa_ctx_set_schedule: bad argument" );
  ctx->schedule = schedule;
  return AA_OK;
}
void * aa_ctx_compute_stream( aa_ctx * ctx ) { return ctx ? ctx->compute : nullptr; }
void * aa_ctx_copy_stream( aa_ctx * ctx ) { return ctx ? ctx->copy : nullptr; }
aa_status aa_ctx_profile( aa_ctx * ctx, int enable )
{
  if ( !ctx ) return fail( AA_ERR_ARGUMENT, "null ctx" );
  if ( !enable ) { (void) hipStreamSynchronize( ctx->compute ); for ( auto ps : ctx->parse_streams ) (void) hipStreamSynchronize( ps ); drain_profile( ctx ); }
  ctx->profile = enable != 0;
  return AA_OK;
}
aa_status aa_ctx_kernel_stats( aa_ctx * ctx, aa_kernel_stats * out, int reset )
{
  if ( !ctx || !out ) return fail( AA_ERR_ARGUMENT, "null argument" );
  HIP_TRY( hipStreamSynchronize( ctx->compute ) );
  for ( auto ps : ctx->parse_streams ) HIP_TRY( hipStreamSynchronize( ps ) );
  drain_profile( ctx );
  ctx->stats.heap_mapped_bytes = ctx->tok.heap_mapped;
  if ( ctx->ws ) {
    int rescued[6] = {};
    HIP_TRY( hipMemcpy( rescued, &ctx->ws->dump[AA_SYNC_WS_RESCUES], sizeof rescued, hipMemcpyDeviceToHost ) );
    ctx->stats.row_handoff_rereads = static_cast<uint64_t>( rescued[0] );
    ctx->stats.row_handoff_stale_polls = static_cast<uint64_t>( rescued[3] );
    ctx->row_handoff_by_kernel[0] = rescued[4]; ctx->row_handoff_by_kernel[1] = rescued[5];
    if ( const char * e = std::getenv( "ALFALFA_AMD_HANDOFF_REPORT" ) ) if ( atoi( e ) )
      std::fprintf( stderr, "alfalfa_amd: row hand-off waits ended by the second look: %d (k_recon_intra4 %d, k_loopfilter_rows4 %d); system-scope load saw it %d, L2 read-modify-write %d; poll repeated still stale %d\n",
                    rescued[0], rescued[4], rescued[5], rescued[1], rescued[2], rescued[3] );
  }
  // (the host lanes' summed parse time comes from their atomic counter: the workers themselves never write to `stats`)
  const uint64_t lanes_us = ctx->host_lanes.parse_us.load();
  ctx->stats.host_batch_parse_cpu_ms = static_cast<double>( lanes_us - ctx->host_lanes.parse_us_mark ) / 1e3;
  *out = ctx->stats;
  if ( reset ) { ctx->stats = aa_kernel_stats {}; ctx->host_lanes.parse_us_mark = lanes_us; }
  return AA_OK;
}

/* ---------------- stream ---------------- */
aa_status aa_stream_create( aa_ctx * ctx, uint16_t width, uint16_t height, aa_stream ** out )
{
  if ( !ctx || !out || !width || !height ) return fail( AA_ERR_ARGUMENT, "aa_stream_create: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  std::unique_ptr<aa_stream> s( new aa_stream( ctx, width, height ) );
  aa_raster_geometry( width, height, &s->pw, &s->ph );
  s->plane_bytes[0] = size_t( s->pw ) * s->ph;
  s->plane_bytes[1] = s->plane_bytes[2] = size_t( s->pw / 2 ) * ( s->ph / 2 );
  s->slot_bytes = align_up( s->plane_bytes[0] + 2 * s->plane_bytes[1] );
  // References(width, height): all three references alias one (blank) raster (decoder.cc:161-169).  Rasters are never written
  // once they are references, so every decoder of this raster size points at the SAME blank one: a decoder that is created
  // long before its first key frame is decoded (a chunk waiting in a pipeline) costs no raster.
  uint8_t * blank = nullptr;
  {
    // (decoders are created from many threads at once; the raster is zero before anybody -- compute or copy stream -- can read it)
    std::lock_guard<std::mutex> g( ctx->blank_mu );
    auto it = ctx->blank.find( s->slot_bytes );
    if ( it != ctx->blank.end() ) blank = it->second;
    else {
      if ( aa_status st = dev_alloc( ctx, s->slot_bytes, &blank ) ) return st;
      hipError_t e = hipMemsetAsync( blank, 0, s->slot_bytes, ctx->compute );
      if ( e == hipSuccess ) e = hipStreamSynchronize( ctx->compute );
      if ( e != hipSuccess ) { dev_free( ctx, blank, s->slot_bytes ); return hip_fail( e, "hipMemsetAsync (blank reference raster)" ); }
      ctx->blank[s->slot_bytes] = blank;
    }
  }
  Slot sl; sl.dev = blank; sl.shared = true;
  s->slots.push_back( sl );
  const int slot = 0;
  for ( int i = 0; i < 3; i++ ) { s->cur_ref_slot[i] = -1; s->cur_ref_frame[i] = -1; }
  for ( int i = 0; i < 3; i++ ) set_ref( s.get(), i, slot, -1 );
  ctx->refs++;
  *out = s.release();
  return AA_OK;
}
void aa_stream_destroy( aa_stream * s )
{
  if ( !s ) return;
  aa_ctx * ctx = s->ctx;
  (void) hipSetDevice( ctx->device );
  hash_drain( ctx );                    // (an outstanding hash call may hold this stream's rasters and fills its Slot caches at the wait)
  // Nothing here waits for the reconstruction stream: what queued kernels may still read or write (rasters, records) goes back
  // to the pools through a release epoch, like everything released while the pipeline runs -- a caller that drops a decoder
  // per chunk does not stall.  What IS waited for: uploads out of this stream's pinned staging (it is handed to other parses),
  // token lanes still on its frames (release_records), header kernels of a two-phase batch that was never launched.
  bool staged = false;
  for ( auto & c : s->chunks ) if ( c.host && c.uploaded ) staged = true;
  if ( staged ) (void) hipStreamSynchronize( ctx->copy );
  for ( auto & f : s->frames ) if ( f.batch && f.batch->hdr_done && !f.enqueued && !f.records_released ) (void) hipEventSynchronize( f.batch->hdr_done );
  for ( auto & f : s->frames ) release_records( s, f, true );
  for ( auto & c : s->chunks ) {
    if ( c.host ) { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->pinned_pool.emplace_back( c.host, c.pinned_bytes ); c.host = nullptr; }
    if ( c.dev ) { dev_free( ctx, c.dev, c.dev_bytes, true ); c.dev = nullptr; }
  }
  for ( auto & sl : s->slots ) if ( sl.dev && !sl.shared ) dev_free_compute( ctx, sl.dev, s->slot_bytes );
  dev_free( ctx, s->dev_segmap, size_t( s->parser.mb_width() ) * s->parser.mb_height(), true );
  delete s;
  if ( --ctx->refs == 0 ) ctx_free( ctx );
}

} // extern "C"
