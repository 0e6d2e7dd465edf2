// runtime.cpp (ABI), its last piece: the serialisation (aa_serialize_batch) -- frames held as records become VP8 frames: the DCT partitions
// written on the device from the records where they lie (serialize_kernels.hip), the frame header and first partition written meanwhile by
// host workers from the macroblock records (serializer.cpp), the frame put together on the host.  The job table goes through the rebase's ring.
namespace {

// What a partition of `rows` macroblock rows can take at most: per macroblock 25 blocks of 16 tokens, a token at most 20 bools (not-end-of-block,
// six tree branches, eleven extra bits, the sign, and the block's end-of-block shared out), a bool at most 7 bits (the range never falls below 1
// of 255: a shift of 7) -- 25 * 16 * 20 * 7 / 8 = 7000 bytes -- and four bytes of flush.
constexpr size_t kSerializeMbBytes = 7000;
size_t serialize_partition_bound( size_t rows, size_t mbw ) { return 16 + rows * mbw * kSerializeMbBytes; }

// the macroblock records of a frame on the host: where the host still has them (a host-parsed or appended frame whose staging was not
// released) they are used in place, else they are copied back as aa_stream_read_records copies them
aa_status serialize_host_records( aa_stream * s, FrameRec & r, std::vector<aa_mb_info> & copy, const aa_mb_info ** out )
{
  if ( r.chunk >= 0 && r.host_job && s->chunks[r.chunk].host ) {
    *out = reinterpret_cast<const aa_mb_info *>( reinterpret_cast<const uint8_t *>( r.host_job ) + align_up( sizeof( aa_dev_frame ) ) );
    return AA_OK;
  }
  aa_dev_frame job;
  HIP_TRY( hipMemcpy( &job, r.dev_job, sizeof job, hipMemcpyDeviceToHost ) );
  copy.resize( r.hdr.num_macroblocks );
  HIP_TRY( hipMemcpy( copy.data(), job.mbs, copy.size() * sizeof( aa_mb_info ), hipMemcpyDeviceToHost ) );
  *out = copy.data();
  return AA_OK;
}

} // namespace

extern "C" {

aa_status aa_parser_last_header_ext( const aa_parser * p, aa_frame_header_ext * out )
{
  if ( !p || !out ) return fail( AA_ERR_ARGUMENT, "aa_parser_last_header_ext: null argument" );
  *out = p->impl.last_header_ext();
  return AA_OK;
}

aa_status aa_stream_last_header_ext( const aa_stream * s, aa_frame_header_ext * out )
{
  if ( !s || !out ) return fail( AA_ERR_ARGUMENT, "aa_stream_last_header_ext: null argument" );
  *out = s->parser.last_header_ext();
  return AA_OK;
}

static aa_status last_sub_modes( const aa::Parser & p, uint8_t * out, size_t capacity, size_t * count, const char * who )
{
  const std::vector<uint8_t> & m = p.last_sub_modes();
  *count = m.size();
  if ( !out ) return AA_OK;
  if ( capacity < m.size() ) return fail( AA_ERR_ARGUMENT, std::string( who ) + ": " + std::to_string( m.size() ) + " sub-block modes, room for " + std::to_string( capacity ) );
  if ( !m.empty() ) std::memcpy( out, m.data(), m.size() );
  return AA_OK;
}
aa_status aa_parser_last_sub_modes( const aa_parser * p, uint8_t * out, size_t capacity, size_t * count )
{
  if ( !p || !count ) return fail( AA_ERR_ARGUMENT, "aa_parser_last_sub_modes: null argument" );
  return last_sub_modes( p->impl, out, capacity, count, "aa_parser_last_sub_modes" );
}
aa_status aa_stream_last_sub_modes( const aa_stream * s, uint8_t * out, size_t capacity, size_t * count )
{
  if ( !s || !count ) return fail( AA_ERR_ARGUMENT, "aa_stream_last_sub_modes: null argument" );
  return last_sub_modes( s->parser, out, capacity, count, "aa_stream_last_sub_modes" );
}

static_assert( sizeof( aa_frame_header_ext ) == 2258, "aa_frame_header_ext is bytes only: the bindings mirror it field by field" );

} // extern "C"

namespace {

// aa_serialize_batch; first_pass (aa_serialize_two_pass_batch, else null): [n][AA_TWO_PASS_UPDATES], the update tables the first pass of a
// two-pass key frame left (aa_encode_two_pass_batch), which an optimising job keeps wherever its own pass makes no update
aa_status serialize_batch( aa_ctx * ctx, aa_serialize_job * jobs, int n, const uint8_t * first_pass )
{
  const auto no = []( aa_status code, int i, const std::string & what ) { return fail( code, "aa_serialize_batch: job " + std::to_string( i ) + ": " + what ); };
  if ( !ctx || !jobs || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_serialize_batch: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  // ---- 1. the arguments: nothing is launched, written or advanced unless every job of the call is good ----
  for ( int i = 0; i < n; i++ ) {
    aa_serialize_job & j = jobs[i];
    if ( !j.stream || !j.hdr || !j.ext || !j.out || ( !j.sub_modes && j.num_sub_modes ) ) return no( AA_ERR_ARGUMENT, i, "null pointer" );
    aa_stream * s = j.stream;
    if ( s->ctx != ctx ) return no( AA_ERR_ARGUMENT, i, "stream belongs to another context" );
    for ( int k = 0; k < i; k++ ) if ( jobs[k].stream == s ) return no( AA_ERR_ARGUMENT, i, "its stream is also job " + std::to_string( k ) + "'s: one frame per stream and call" );
    if ( j.frame_index < 0 || j.frame_index >= static_cast<int>( s->frames.size() ) ) return no( AA_ERR_ARGUMENT, i, "frame index out of range" );
    if ( s->frames[j.frame_index].records_released ) return no( AA_ERR_ARGUMENT, i, "the frame's records were released" );
    const unsigned parts = j.hdr->num_dct_partitions;
    if ( parts != 1 && parts != 2 && parts != 4 && parts != 8 ) return no( AA_ERR_ARGUMENT, i, "num_dct_partitions is " + std::to_string( parts ) + ": a frame has 1, 2, 4 or 8 DCT partitions" );
    if ( j.advance_state && j.probs_before ) return no( AA_ERR_ARGUMENT, i, "advance_state together with probs_before: the stream's state can only follow a frame coded against it" );
    if ( j.advance_state && ( j.ext->color_space || j.ext->clamping_type || j.ext->filter_type ) )
      return no( AA_ERR_ARGUMENT, i, "advance_state with color_space, clamping_type or filter_type set: the decoder refuses such a frame and no state follows it" );
    const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
    if ( j.hdr->mb_width != s->parser.mb_width() || j.hdr->mb_height != s->parser.mb_height() || j.hdr->num_macroblocks != nmb
         || j.hdr->width != s->parser.width() || j.hdr->height != s->parser.height() )
      return no( AA_ERR_ARGUMENT, i, "the header's dimensions are not this decoder's" );
    if ( j.capacity > 0xFFFFFFFFu ) return no( AA_ERR_ARGUMENT, i, "capacity beyond 4 GiB" );
    j.size = 0;
  }

  const double t_call = now_ms();
  // ---- 2. every frame's records final and in HBM; the macroblock records on the host ----
  std::vector<std::vector<aa_mb_info>> mb_copies( n );
  std::vector<const aa_mb_info *> mbs( n, nullptr );
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = jobs[i].stream;
    FrameRec & r = s->frames[jobs[i].frame_index];
    if ( aa_status st = resolve_summary( s, r ) ) return st;
    if ( aa_status st = aa_stream_upload( s ) ) return st;          // (the compute stream waits for the copy)
    if ( jobs[i].advance_state ) if ( aa_status st = segmap_to_host( s ) ) return st;
  }
  HIP_TRY( hipStreamSynchronize( ctx->copy ) );
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = jobs[i].stream;
    FrameRec & r = s->frames[jobs[i].frame_index];
    if ( r.hdr.mb_width != jobs[i].hdr->mb_width || r.hdr.mb_height != jobs[i].hdr->mb_height ) return no( AA_ERR_LOGIC, i, "the frame's records are of another size" );
    if ( aa_status st = serialize_host_records( s, r, mb_copies[i], &mbs[i] ) ) return st;
  }

  // ---- 3. the job table (tables the tokens are coded with), the lane list, the staging piece ----
  std::vector<aa::ProbTables> tables( n );
  std::vector<aa_frame_header_ext> exts( n );          // the headers as they are written: the callers' (optimise: with the passes' fields) -- handed back on success
  bool any_optimise = false;
  uint32_t max_mbs = 0;
  std::vector<size_t> out_off( n );
  std::vector<uint32_t> region( n );
  size_t staging_total = 0, n_lanes = 0;
  for ( int i = 0; i < n; i++ ) {
    const aa_serialize_job & j = jobs[i];
    uint8_t before[1101];
    if ( j.probs_before ) std::memcpy( before, j.probs_before, 1101 );
    else {
      const aa::ProbTables & t = j.stream->parser.probs();
      std::memcpy( before, t.coeff, 1056 ); std::memcpy( before + 1056, t.y_mode, 4 ); std::memcpy( before + 1060, t.uv_mode, 3 ); std::memcpy( before + 1063, t.mv, 38 );
    }
    exts[i] = *j.ext;
    if ( j.optimise ) {            // the passes decide the token updates: the table the kernels start from is the one before the frame
      std::memset( exts[i].token_prob_update, 0, sizeof exts[i].token_prob_update ); std::memset( exts[i].token_prob, 0, sizeof exts[i].token_prob );
      any_optimise = true;
      max_mbs = std::max<uint32_t>( max_mbs, j.hdr->num_macroblocks );
    }
    aa::frame_probs( before, j.hdr->key_frame != 0, exts[i], tables[i] );
    const unsigned parts = j.hdr->num_dct_partitions;
    const size_t rows = ( j.hdr->mb_height + parts - 1 ) / parts;      // (partition 0 has the most rows)
    region[i] = static_cast<uint32_t>( align_up( std::min<size_t>( std::max<size_t>( j.capacity, 16 ), serialize_partition_bound( rows, j.hdr->mb_width ) ), 16 ) );
    out_off[i] = staging_total;
    staging_total += size_t( region[i] ) * parts;
    n_lanes += parts;
  }
  const size_t table_bytes = align_up( size_t( n ) * sizeof( aa_serialize_dev_job ) ), lanes_bytes = align_up( n_lanes * sizeof( uint32_t ) );
  const size_t sizes_bytes = align_up( size_t( n ) * 8 * sizeof( uint32_t ) );
  const size_t counts_bytes = any_optimise ? align_up( size_t( n ) * AA_SERIALIZE_COUNTS * sizeof( uint32_t ) ) : 0, updates_bytes = any_optimise ? align_up( size_t( n ) * AA_SERIALIZE_UPDATES ) : 0;
  const size_t first_bytes = first_pass && any_optimise ? align_up( size_t( n ) * AA_TWO_PASS_UPDATES ) : 0;
  const size_t up_bytes = table_bytes + lanes_bytes + first_bytes, piece_bytes = up_bytes + sizes_bytes + counts_bytes + updates_bytes + align_up( staging_total );
  JobRing::Entry * rb = nullptr;
  if ( aa_status st = ctx->rebase_ring.take( up_bytes, align_up( 64 * sizeof( aa_rebase_dev_job ) ), &rb ) ) return st;
  uint8_t * piece = nullptr;
  if ( aa_status st = dev_alloc_compute( ctx, piece_bytes, &piece ) ) return st;
  struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { dev_free_compute( c, p, b ); } } back { ctx, piece, piece_bytes };
  aa_serialize_dev_job * table = reinterpret_cast<aa_serialize_dev_job *>( rb->host );
  uint32_t * lanes = reinterpret_cast<uint32_t *>( rb->host + table_bytes );
  uint8_t * const dev_sizes = piece + up_bytes, * const dev_counts = dev_sizes + sizes_bytes, * const dev_updates = dev_counts + counts_bytes, * const dev_staging = dev_updates + updates_bytes;
  size_t lane = 0;
  for ( int i = 0; i < n; i++ ) {
    aa_serialize_dev_job & d = table[i];
    std::memset( &d, 0, sizeof d );
    d.frame = jobs[i].stream->frames[jobs[i].frame_index].dev_job;
    d.out = dev_staging + out_off[i];
    d.sizes = reinterpret_cast<uint32_t *>( dev_sizes ) + size_t( i ) * 8;
    d.region = region[i]; d.nparts = jobs[i].hdr->num_dct_partitions;
    d.optimise = jobs[i].optimise != 0;
    d.skip_enabled = d.optimise || exts[i].skip_enabled != 0;          // (optimize_prob_skip always sets prob_skip_false)
    if ( d.optimise ) { d.counts = reinterpret_cast<uint32_t *>( dev_counts ) + size_t( i ) * AA_SERIALIZE_COUNTS; d.updates = dev_updates + size_t( i ) * AA_SERIALIZE_UPDATES; }
    if ( d.optimise && first_bytes ) d.first_pass = piece + table_bytes + lanes_bytes + size_t( i ) * AA_TWO_PASS_UPDATES;
    std::memcpy( d.probs, tables[i].coeff, 1056 );
    for ( unsigned p = 0; p < d.nparts; p++ ) lanes[lane++] = static_cast<uint32_t>( i ) << 3 | p;
  }
  if ( first_bytes ) std::memcpy( rb->host + table_bytes + lanes_bytes, first_pass, size_t( n ) * AA_TWO_PASS_UPDATES );
  // a wave is bound by its instruction issue and its lanes diverge: every SIMD gets a wave before any wave gets a second lane
  int cus = 0;
  const int simds = hipDeviceGetAttribute( &cus, hipDeviceAttributeMultiprocessorCount, ctx->device ) == hipSuccess && cus > 0 ? 4 * cus : 1024;
  const int lanes_per_wave = static_cast<int>( std::min<size_t>( 64, ( n_lanes + simds - 1 ) / simds ) );

  hipEvent_t ev[3] = { get_event( ctx ), get_event( ctx ), get_event( ctx ) };
  struct Events { aa_ctx * c; hipEvent_t * e; ~Events() { for ( int i = 0; i < 3; i++ ) if ( e[i] ) c->free_events.push_back( e[i] ); } } events { ctx, ev };
  if ( !ev[0] || !ev[1] || !ev[2] ) return fail( AA_ERR_HIP, "aa_serialize_batch: hipEventCreate failed" );
  HIP_TRY( hipEventRecord( ev[0], ctx->compute ) );
  HIP_TRY( hipMemcpyAsync( piece, rb->host, up_bytes, hipMemcpyHostToDevice, ctx->compute ) );
  if ( aa_status st = ctx->rebase_ring.mark( *rb, ctx->compute ) ) return st;
  HIP_TRY( hipMemsetAsync( dev_sizes, 0, sizes_bytes + counts_bytes + updates_bytes, ctx->compute ) );
  // ---- 3a. optimise: counts and probabilities first; what the header needs of them comes to the host in one small copy, in front of the token kernel ----
  size_t updates_pinned = 0;
  uint8_t * updates_host = nullptr;
  struct Unpin { aa_ctx * c; uint8_t * p; size_t b; ~Unpin() { if ( p ) { std::lock_guard<std::mutex> g( c->pool_mu ); c->pinned_pool.emplace_back( p, b ); } } };
  hipEvent_t ev_probs = nullptr;
  if ( any_optimise ) {
    updates_host = pinned_get( ctx, updates_bytes, &updates_pinned );
    ev_probs = get_event( ctx );
    if ( !updates_host || !ev_probs ) return fail( AA_ERR_HIP, "aa_serialize_batch: pinned staging allocation failed" );
    if ( int e = aa::launch_serialize_probs( reinterpret_cast<aa_serialize_dev_job *>( piece ), n, max_mbs, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_token_counts / k_token_probs" );
    HIP_TRY( hipMemcpyAsync( updates_host, dev_updates, updates_bytes, hipMemcpyDeviceToHost, ctx->compute ) );
    HIP_TRY( hipEventRecord( ev_probs, ctx->compute ) );
  }
  Unpin unpin_updates { ctx, updates_host, updates_pinned };
  struct EvBack { aa_ctx * c; hipEvent_t e; ~EvBack() { if ( e ) c->free_events.push_back( e ); } } ev_back { ctx, ev_probs };
  if ( int e = aa::launch_serialize_tokens( reinterpret_cast<const aa_serialize_dev_job *>( piece ), reinterpret_cast<const uint32_t *>( piece + table_bytes ), static_cast<int>( n_lanes ),
                                            lanes_per_wave, ctx->compute ) )
    return hip_fail( static_cast<hipError_t>( e ), "k_serialize_tokens" );
  HIP_TRY( hipEventRecord( ev[1], ctx->compute ) );

  // ---- 4. meanwhile on the host, a worker per job at a time: frame header + first partition ----
  if ( any_optimise ) {
    HIP_TRY( hipEventSynchronize( ev_probs ) );
    for ( int i = 0; i < n; i++ ) {
      if ( !jobs[i].optimise ) continue;
      const uint8_t * u = updates_host + size_t( i ) * AA_SERIALIZE_UPDATES;
      aa_frame_header_ext & x = exts[i];
      std::memcpy( x.token_prob_update, u, 1056 ); std::memcpy( x.token_prob, u + 1056, 1056 );      // optimize_probability_tables
      x.skip_enabled = 1; x.prob_skip_false = u[2112];                                                 // optimize_prob_skip
      if ( !jobs[i].hdr->key_frame ) {                                                                   // optimize_interframe_probs: only what is > 0
        if ( u[2113] ) x.prob_inter = u[2113];
        if ( u[2114] ) x.prob_references_last = u[2114];
        if ( u[2115] ) x.prob_references_golden = u[2115];
      }
    }
  }
  std::vector<uint32_t> counts_host;
  for ( int i = 0; i < n; i++ ) if ( jobs[i].optimise && jobs[i].counts_out && counts_host.empty() ) {
    counts_host.resize( size_t( n ) * AA_SERIALIZE_COUNTS );
    HIP_TRY( hipMemcpy( counts_host.data(), dev_counts, counts_host.size() * sizeof( uint32_t ), hipMemcpyDeviceToHost ) );     // (final since ev_probs)
  }
  const double t_first = now_ms();
  std::vector<std::vector<uint8_t>> first( n );
  std::vector<aa_status> status( n, AA_OK );
  std::vector<std::string> message( n );
  {
    std::atomic<int> next { 0 };
    auto work = [&]() {
      for ( ;; ) {
        const int i = next.fetch_add( 1 );
        if ( i >= n ) return;
        try { aa::write_first_partition( *jobs[i].hdr, exts[i], tables[i], mbs[i], jobs[i].sub_modes, jobs[i].num_sub_modes, first[i] ); }
        catch ( const aa::ParseError & e ) { status[i] = e.code; message[i] = e.message; }
      }
    };
    const int workers = std::max( 1, std::min( worker_threads( 0 ), n ) );
    if ( workers == 1 ) work();
    else {
      std::vector<std::thread> pool;
      for ( int t = 0; t < workers; t++ ) pool.emplace_back( work );
      for ( auto & t : pool ) t.join();
    }
  }
  const double ms_first = now_ms() - t_first;

  // ---- 5. the partitions' sizes, then the partitions that fitted, down ----
  size_t pinned_bytes = 0;
  uint8_t * sizes_host = pinned_get( ctx, sizes_bytes, &pinned_bytes );
  if ( !sizes_host ) return fail( AA_ERR_HIP, "aa_serialize_batch: pinned staging allocation failed" );
  Unpin unpin_sizes { ctx, sizes_host, pinned_bytes };
  HIP_TRY( hipMemcpyAsync( sizes_host, dev_sizes, sizes_bytes, hipMemcpyDeviceToHost, ctx->compute ) );
  HIP_TRY( hipStreamSynchronize( ctx->compute ) );
  if ( aa_status st = check_watchdog( ctx ) ) return st;
  for ( int i = 0; i < n; i++ ) if ( status[i] != AA_OK ) return no( status[i], i, message[i] );
  const uint32_t * sizes = reinterpret_cast<const uint32_t *>( sizes_host );
  // the frames' sizes; a refusal names the first frame that does not fit
  std::vector<size_t> part_off( size_t( n ) * 8, 0 );
  size_t down_total = 0;
  for ( int i = 0; i < n; i++ ) {
    const unsigned parts = jobs[i].hdr->num_dct_partitions;
    size_t total = ( jobs[i].hdr->key_frame ? 10u : 3u ) + first[i].size() + 3u * ( parts - 1 );
    for ( unsigned p = 0; p < parts; p++ ) { total += sizes[i * 8 + p]; part_off[size_t( i ) * 8 + p] = down_total; down_total += align_up( sizes[i * 8 + p], 16 ); }
    jobs[i].size = total;
  }
  for ( int i = 0; i < n; i++ )
    if ( jobs[i].size > jobs[i].capacity ) {
      const size_t need = jobs[i].size, room = jobs[i].capacity;
      for ( int k = 0; k < n; k++ ) jobs[k].size = 0;
      return no( AA_ERR_ARGUMENT, i, "output buffer too small: " + std::to_string( need ) + " bytes needed, room for " + std::to_string( room ) );
    }
  // (every partition is within its range now: a frame that fits its capacity has no partition beyond min( capacity, worst case ))
  size_t down_pinned = 0;
  uint8_t * down = pinned_get( ctx, std::max<size_t>( down_total, 16 ), &down_pinned );
  if ( !down ) return fail( AA_ERR_HIP, "aa_serialize_batch: pinned staging allocation failed" );
  Unpin unpin_down { ctx, down, down_pinned };
  for ( int i = 0; i < n; i++ )
    for ( unsigned p = 0; p < jobs[i].hdr->num_dct_partitions; p++ ) {
      const uint32_t bytes = sizes[i * 8 + p];
      if ( bytes > region[i] ) return no( AA_ERR_LOGIC, i, "a partition that fits its frame's capacity lies outside its staging range" );
      if ( bytes ) HIP_TRY( hipMemcpyAsync( down + part_off[size_t( i ) * 8 + p], dev_staging + out_off[i] + size_t( p ) * region[i], bytes, hipMemcpyDeviceToHost, ctx->compute ) );
    }
  HIP_TRY( hipEventRecord( ev[2], ctx->compute ) );
  HIP_TRY( hipStreamSynchronize( ctx->compute ) );
  float ms_kernel = 0, ms_down = 0;
  (void) hipEventElapsedTime( &ms_kernel, ev[0], ev[1] ); (void) hipEventElapsedTime( &ms_down, ev[1], ev[2] );

  // ---- 6. the frames put together in the callers' buffers; then the states that follow their frames ----
  const double t_assemble = now_ms();
  // (a frame is assembled and parsed in a buffer of the call's own, by a COPY of its stream's parser: `out` is written and the state
  // committed only when every frame of the call that is to advance a state has parsed)
  std::vector<std::vector<uint8_t>> built( n );
  std::vector<std::unique_ptr<aa::Parser>> advanced( n );
  {
    std::atomic<int> next { 0 };
    auto work = [&]() {
      for ( ;; ) {
        const int i = next.fetch_add( 1 );
        if ( i >= n ) return;
        const uint8_t * ptr[8];
        for ( unsigned p = 0; p < 8; p++ ) ptr[p] = down + part_off[size_t( i ) * 8 + p];
        built[i].resize( jobs[i].size );
        aa::assemble_frame( *jobs[i].hdr, first[i], ptr, sizes + size_t( i ) * 8, built[i].data(), built[i].size() );
        if ( !jobs[i].advance_state ) continue;
        // exactly what parsing the frame does to a DecoderState: it is parsed (records into scratch)
        aa_stream * s = jobs[i].stream;
        const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
        std::vector<aa_mb_info> scratch_mb( nmb );
        std::vector<int16_t> scratch_cf( nmb * 25 * 16 );
        aa_frame_header h;
        advanced[i].reset( new aa::Parser( s->parser ) );
        try { advanced[i]->parse( built[i].data(), built[i].size(), h, scratch_mb.data(), scratch_cf.data() ); }
        catch ( const aa::ParseError & e ) { status[i] = e.code; message[i] = "the written frame does not parse: " + e.message; }
      }
    };
    const int workers = std::max( 1, std::min( worker_threads( 0 ), n ) );
    if ( workers == 1 ) work();
    else {
      std::vector<std::thread> pool;
      for ( int t = 0; t < workers; t++ ) pool.emplace_back( work );
      for ( auto & t : pool ) t.join();
    }
  }
  for ( int i = 0; i < n; i++ ) if ( status[i] != AA_OK ) { for ( int k = 0; k < n; k++ ) jobs[k].size = 0; return no( status[i], i, message[i] ); }
  for ( int i = 0; i < n; i++ ) {
    std::memcpy( jobs[i].out, built[i].data(), built[i].size() );
    if ( advanced[i] ) jobs[i].stream->parser = *advanced[i];
    *jobs[i].ext = exts[i];
    if ( jobs[i].optimise && jobs[i].counts_out ) std::memcpy( jobs[i].counts_out, counts_host.data() + size_t( i ) * AA_SERIALIZE_COUNTS, AA_SERIALIZE_COUNTS * sizeof( uint32_t ) );
  }
  const double t_end = now_ms();
  const double timing[5] = { t_end - t_call, ms_kernel, ms_down, ms_first, t_end - t_assemble };
  std::memcpy( ctx->serialize_timing, timing, sizeof timing );
  return AA_OK;
}

} // namespace

extern "C" {

aa_status aa_serialize_batch( aa_ctx * ctx, aa_serialize_job * jobs, int n ) { return serialize_batch( ctx, jobs, n, nullptr ); }
aa_status aa_serialize_two_pass_batch( aa_ctx * ctx, aa_serialize_job * jobs, int n, const uint8_t * first_pass_updates )
{
  if ( !first_pass_updates ) return fail( AA_ERR_ARGUMENT, "aa_serialize_two_pass_batch: null argument" );
  return serialize_batch( ctx, jobs, n, first_pass_updates );
}

aa_status aa_serialize_host( const aa_frame_header * hdr, const aa_frame_header_ext * ext, const uint8_t * probs_before, const aa_mb_info * mbs,
                             const int16_t * coeffs, const uint8_t * sub_modes, size_t num_sub_modes, uint8_t * out, size_t capacity, size_t * size )
{
  if ( !hdr || !ext || !mbs || !out || !size || ( !probs_before && !hdr->key_frame ) || ( !sub_modes && num_sub_modes ) ) return fail( AA_ERR_ARGUMENT, "aa_serialize_host: null argument" );
  if ( hdr->num_coeff_blocks && !coeffs ) return fail( AA_ERR_ARGUMENT, "aa_serialize_host: coefficient blocks missing" );
  if ( hdr->num_macroblocks != uint32_t( hdr->mb_width ) * hdr->mb_height ) return fail( AA_ERR_ARGUMENT, "aa_serialize_host: the header's macroblock count is not its dimensions'" );
  for ( uint32_t i = 0; i < hdr->num_macroblocks; i++ ) {
    const uint32_t nblk = static_cast<uint32_t>( __builtin_popcount( mbs[i].nz_mask & 0x1FFFFFFu ) );
    if ( ( mbs[i].nz_mask >> 25 ) || ( nblk && size_t( mbs[i].coeff_index ) + nblk > hdr->num_coeff_blocks ) )
      return fail( AA_ERR_ARGUMENT, "aa_serialize_host: macroblock " + std::to_string( i ) + " points outside the coefficient blocks" );
  }
  std::vector<uint8_t> frame;
  try { aa::serialize_frame_host( *hdr, *ext, probs_before, mbs, coeffs, sub_modes, num_sub_modes, frame ); }
  catch ( const aa::ParseError & e ) { return fail( e.code, e.message ); }
  *size = frame.size();
  if ( frame.size() > capacity ) return fail( AA_ERR_ARGUMENT, "aa_serialize_host: output buffer too small: " + std::to_string( frame.size() ) + " bytes needed, room for " + std::to_string( capacity ) );
  std::memcpy( out, frame.data(), frame.size() );
  return AA_OK;
}

aa_status aa_serialize_last_timing( aa_ctx * ctx, double out[5] )
{
  if ( !ctx || !out ) return fail( AA_ERR_ARGUMENT, "aa_serialize_last_timing: null argument" );
  std::memcpy( out, ctx->serialize_timing, sizeof ctx->serialize_timing );
  return AA_OK;
}

} // extern "C"
