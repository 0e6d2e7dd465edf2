// runtime.cpp (ABI), its last piece: the rebase (aa_rebase_batch) -- inter frames' residues recomputed against the job streams' current
// references on the device, the records built on the host and appended as aa_stream_append_records appends them; kernels in
// rebase_kernels.hip.  And aa_quant_factors, the quantiser of a new frame's header.
namespace {

// The call's dense scratch (AA_REBASE_MB_BYTES per macroblock) is bounded: a call whose jobs would take more than a 64th of the
// context's memory limit, and never more than 256 MiB, works through them in slices (ALFALFA_AMD_REBASE_SLICE_BYTES: tests).
size_t rebase_slice_bytes( const aa_ctx * ctx )
{
  if ( const char * e = std::getenv( "ALFALFA_AMD_REBASE_SLICE_BYTES" ) ) return static_cast<size_t>( std::max( 1ll, atoll( e ) ) );
  return std::min( ctx->pool_soft_limit / 64, size_t( 256 ) << 20 );
}

struct RebaseCounts { uint32_t blocks = 0, intra = 0; };

// A job's records from what the kernels left: stored blocks in parse order (Y2 if present, then 0..23 ascending), flags as the
// parser sets them for the serialised frame (every rebased frame codes mb_skip_coeff = no coefficient left: encoder.cc:442-457,632-657).
// coeffs_out == nullptr: count only.
RebaseCounts rebase_records( const aa_mb_info * in, const uint32_t * masks, const int16_t * dense, size_t nmb, aa_mb_info * out, int16_t * coeffs_out )
{
  RebaseCounts c;
  for ( size_t i = 0; i < nmb; i++ ) {
    const bool inter = in[i].ref_frame != 0;
    const bool has_y2 = in[i].y_mode != 4 /* B_PRED */ && in[i].y_mode != 9 /* SPLITMV */;
    const uint32_t mask = masks[i] & ( has_y2 ? 0x1FFFFFFu : 0xFFFFFFu );
    if ( !inter ) c.intra++;
    if ( out ) {
      aa_mb_info & m = out[i];
      m = in[i];
      m.reserved = 0;
      m.flags = static_cast<uint8_t>( ( inter ? AA_MB_INTER : 0u ) | ( has_y2 ? AA_MB_HAS_Y2 : 0u )
                                      | ( mask ? AA_MB_HAS_NONZERO : AA_MB_SKIP | ( has_y2 ? AA_MB_LF_SKIP_INNER : 0u ) ) );
      m.nz_mask = mask; m.coeff_index = c.blocks;
    }
    if ( coeffs_out && mask ) {
      const int16_t * src = dense + i * ( AA_REBASE_MB_BYTES / 2 );
      int16_t * dst = coeffs_out + size_t( c.blocks ) * 16;
      if ( mask >> 24 ) { std::memcpy( dst, src + 24 * 16, 32 ); dst += 16; }
      for ( int b = 0; b < 24; b++ ) if ( ( mask >> b ) & 1u ) { std::memcpy( dst, src + b * 16, 32 ); dst += 16; }
    }
    c.blocks += static_cast<uint32_t>( __builtin_popcount( mask ) );
  }
  return c;
}

} // namespace

extern "C" {

/* Quantizer::Quantizer( QuantIndices ) (quantization.cc:83-93): the factors {y_dc, y_ac, y2_dc, y2_ac, uv_dc, uv_ac} of a frame header
 * whose base index is y_ac_qi and whose deltas are {y_dc, y2_dc, y2_ac, uv_dc, uv_ac} (NULL: none). */
void aa_quant_factors( int y_ac_qi, const int8_t deltas[5], uint16_t out[6] )
{
  int d[5] = { 0, 0, 0, 0, 0 };
  if ( deltas ) for ( int i = 0; i < 5; i++ ) d[i] = deltas[i];
  aa::quant_factors( y_ac_qi, d, out );
}

aa_status aa_rebase_batch( aa_ctx * ctx, aa_rebase_job * jobs, int n )
{
  const auto no = []( aa_status code, int i, const std::string & what ) { return fail( code, "aa_rebase_batch: job " + std::to_string( i ) + ": " + what ); };
  if ( !ctx || !jobs || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_rebase_batch: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  // ---- 1. the arguments: nothing is launched, nothing appended unless every job of the call is good ----
  for ( int i = 0; i < n; i++ ) {
    aa_rebase_job & j = jobs[i];
    if ( !j.stream || !j.hdr || !j.mbs || !j.mbs_out || !j.target.y || !j.target.u || !j.target.v ) return no( AA_ERR_ARGUMENT, i, "null pointer" );
    if ( !j.coeffs_out && j.coeff_capacity_blocks ) return no( AA_ERR_ARGUMENT, i, "null pointer" );
    aa_stream * s = j.stream;
    if ( s->ctx != ctx ) return no( AA_ERR_ARGUMENT, i, "stream belongs to another context" );
    for ( int k = 0; k < i; k++ ) if ( jobs[k].stream == s ) return no( AA_ERR_ARGUMENT, i, "its stream is also job " + std::to_string( k ) + "'s: one new frame per stream and call" );
    if ( j.hdr->key_frame ) return no( AA_ERR_ARGUMENT, i, "the new frame's header says key frame: a rebase makes inter frames" );
    if ( j.hdr->segmentation_enabled )
      return no( AA_ERR_UNSUPPORTED, i, "segmentation is enabled: the rebase quantises with the frame quantiser only (reencode.cc:274) and the frame would not decode to what was reconstructed" );
    const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
    if ( j.hdr->mb_width != s->parser.mb_width() || j.hdr->mb_height != s->parser.mb_height() || j.hdr->num_macroblocks != nmb )
      return no( AA_ERR_ARGUMENT, i, "the header's macroblock dimensions are not this decoder's" );
    if ( s->next_submit != static_cast<int>( s->frames.size() ) ) return no( AA_ERR_LOGIC, i, "its stream holds a frame that is appended but not decoded: the references are not current" );
    if ( j.target.y_stride < int64_t( s->pw ) || j.target.uv_stride < int64_t( s->pw / 2 ) ) return no( AA_ERR_ARGUMENT, i, "row stride smaller than the padded plane's width" );
    for ( int f = 0; f < 6; f++ ) if ( !j.hdr->quant[0][f] ) return no( AA_ERR_ARGUMENT, i, "a quantiser factor of the header is zero" );
    for ( size_t m = 0; m < nmb; m++ ) {
      const aa_mb_info & mb = j.mbs[m];
      if ( mb.y_mode > 9 || mb.uv_mode > 3 || mb.ref_frame > 3 || mb.segment_id > 3 || mb.lf_level > 63 || ( mb.ref_frame == 0 ) != ( mb.y_mode <= 4 ) )
        return no( AA_ERR_ARGUMENT, i, "macroblock " + std::to_string( m ) + " has a field out of range" );
      if ( mb.y_mode == 4 ) for ( int b = 0; b < 16; b++ ) if ( mb.u.b_mode[b] > 9 ) return no( AA_ERR_ARGUMENT, i, "macroblock " + std::to_string( m ) + " has a field out of range" );
    }
    for ( int r = 0; r < 3; r++ ) if ( s->cur_ref_slot[r] < 0 || !s->slots[s->cur_ref_slot[r]].dev ) return no( AA_ERR_LOGIC, i, "its stream has no reference rasters" );
    j.num_coeff_blocks = 0; j.frame_index = -1;
  }

  const double t_call = now_ms();
  double ms_kernels = 0, ms_download = 0, ms_records = 0;
  // ---- 2..5. slice by slice: job table and records up, the two kernels, coefficients and masks down, records into the caller's arrays ----
  const size_t share = rebase_slice_bytes( ctx );
  std::vector<uint32_t> intra_mbs( n, 0 );
  for ( int first = 0; first < n; ) {
    int count = 0;
    size_t dense_total = 0, masks_total = 0, records_total = 0, raster_total = 0;
    uint32_t max_mbs = 0;
    while ( first + count < n ) {
      const aa_stream * s = jobs[first + count].stream;
      const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
      if ( count && dense_total + nmb * AA_REBASE_MB_BYTES > share ) break;
      dense_total += align_up( nmb * AA_REBASE_MB_BYTES ); masks_total += align_up( nmb * sizeof( uint32_t ) );
      records_total += align_up( nmb * sizeof( aa_mb_info ) );
      raster_total += s->slot_bytes;
      max_mbs = std::max<uint32_t>( max_mbs, static_cast<uint32_t>( nmb ) );
      count++;
    }
    // the pinned side: job table | every job's input records (a JobRing entry, read by one copy); the device piece: the same, then masks |
    // dense coefficients | reconstruction rasters; the results' pinned staging: masks | dense coefficients of every job
    const size_t table_bytes = align_up( size_t( count ) * sizeof( aa_rebase_dev_job ) );
    const size_t up_bytes = table_bytes + records_total, result_bytes = masks_total + dense_total;
    const size_t piece_bytes = up_bytes + result_bytes + raster_total;
    JobRing::Entry * rb = nullptr;
    if ( aa_status st = ctx->rebase_ring.take( up_bytes, align_up( 64 * sizeof( aa_rebase_dev_job ) ), &rb ) ) return st;
    uint8_t * piece = nullptr;
    if ( aa_status st = dev_alloc_compute( ctx, piece_bytes, &piece ) ) return st;
    struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { dev_free_compute( c, p, b ); } } back { ctx, piece, piece_bytes };
    size_t staging_bytes = 0;
    uint8_t * staging = pinned_get( ctx, result_bytes, &staging_bytes );
    if ( !staging ) return fail( AA_ERR_HIP, "aa_rebase_batch: pinned staging allocation failed" );
    struct Unpin { aa_ctx * c; uint8_t * p; size_t b; ~Unpin() { std::lock_guard<std::mutex> g( c->pool_mu ); c->pinned_pool.emplace_back( p, b ); } } unpin { ctx, staging, staging_bytes };

    aa_rebase_dev_job * table = reinterpret_cast<aa_rebase_dev_job *>( rb->host );
    std::vector<size_t> result_off( count );
    size_t up_off = table_bytes, res_off = 0, raster_off = up_bytes + result_bytes;
    bool any_intra = false;
    for ( int k = 0; k < count; k++ ) {
      const aa_rebase_job & j = jobs[first + k];
      aa_stream * s = j.stream;
      const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
      aa_rebase_dev_job & d = table[k];
      std::memset( &d, 0, sizeof d );
      for ( int r = 0; r < 3; r++ ) for ( int p = 0; p < 3; p++ ) d.ref[1 + r][p] = slot_plane( s, s->cur_ref_slot[r], p );
      d.target[0] = static_cast<const uint8_t *>( j.target.y ); d.target[1] = static_cast<const uint8_t *>( j.target.u ); d.target[2] = static_cast<const uint8_t *>( j.target.v );
      d.target_stride[0] = j.target.y_stride; d.target_stride[1] = j.target.uv_stride;
      uint8_t * raster = piece + raster_off;
      d.recon[0] = raster; d.recon[1] = raster + s->plane_bytes[0]; d.recon[2] = raster + s->plane_bytes[0] + s->plane_bytes[1];
      raster_off += s->slot_bytes;
      std::memcpy( rb->host + up_off, j.mbs, nmb * sizeof( aa_mb_info ) );
      d.mbs = reinterpret_cast<const aa_mb_info *>( piece + up_off );
      up_off += align_up( nmb * sizeof( aa_mb_info ) );
      result_off[k] = res_off;
      d.masks = reinterpret_cast<uint32_t *>( piece + up_bytes + res_off );
      d.coeffs = reinterpret_cast<int16_t *>( piece + up_bytes + res_off + align_up( nmb * sizeof( uint32_t ) ) );
      res_off += align_up( nmb * sizeof( uint32_t ) ) + align_up( nmb * AA_REBASE_MB_BYTES );
      std::memcpy( d.quant, j.hdr->quant[0], sizeof d.quant );
      d.mbw = j.hdr->mb_width; d.mbh = j.hdr->mb_height;
      for ( size_t m = 0; m < nmb && !d.has_intra; m++ ) if ( j.mbs[m].ref_frame == 0 ) d.has_intra = 1;
      any_intra = any_intra || d.has_intra;
    }
    hipEvent_t ev[3] = { get_event( ctx ), get_event( ctx ), get_event( ctx ) };      // (aa_rebase_last_timing: table up + kernels, results down)
    struct Events { aa_ctx * c; hipEvent_t * e; ~Events() { for ( int i = 0; i < 3; i++ ) if ( e[i] ) c->free_events.push_back( e[i] ); } } events { ctx, ev };
    if ( !ev[0] || !ev[1] || !ev[2] ) return fail( AA_ERR_HIP, "aa_rebase_batch: hipEventCreate failed" );
    HIP_TRY( hipEventRecord( ev[0], ctx->compute ) );
    HIP_TRY( hipMemcpyAsync( piece, rb->host, up_bytes, hipMemcpyHostToDevice, ctx->compute ) );
    if ( aa_status st = ctx->rebase_ring.mark( *rb, ctx->compute ) ) return st;
    if ( int e = aa::launch_rebase( reinterpret_cast<const aa_rebase_dev_job *>( piece ), count, max_mbs, any_intra, ctx->compute ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_rebase_inter / k_rebase_intra" );
    HIP_TRY( hipEventRecord( ev[1], ctx->compute ) );
    HIP_TRY( hipMemcpyAsync( staging, piece + up_bytes, result_bytes, hipMemcpyDeviceToHost, ctx->compute ) );
    HIP_TRY( hipEventRecord( ev[2], ctx->compute ) );
    HIP_TRY( hipStreamSynchronize( ctx->compute ) );
    if ( aa_status st = check_watchdog( ctx ) ) return st;
    { float a = 0, b = 0; if ( hipEventElapsedTime( &a, ev[0], ev[1] ) == hipSuccess && hipEventElapsedTime( &b, ev[1], ev[2] ) == hipSuccess ) { ms_kernels += a; ms_download += b; } }
    const double t_records = now_ms();

    // records, one host worker per job at a time; a job whose coefficient array is too small stops the call
    std::atomic<int> next { 0 }, short_job { -1 };
    auto work = [&]() {
      for ( ;; ) {
        const int k = next.fetch_add( 1 );
        if ( k >= count ) return;
        aa_rebase_job & j = jobs[first + k];
        const size_t nmb = size_t( j.hdr->mb_width ) * j.hdr->mb_height;
        const uint32_t * masks = reinterpret_cast<const uint32_t *>( staging + result_off[k] );
        const int16_t * dense = reinterpret_cast<const int16_t *>( staging + result_off[k] + align_up( nmb * sizeof( uint32_t ) ) );
        const RebaseCounts need = rebase_records( j.mbs, masks, dense, nmb, nullptr, nullptr );
        j.num_coeff_blocks = need.blocks; intra_mbs[first + k] = need.intra;
        if ( need.blocks > j.coeff_capacity_blocks ) { int none = -1; short_job.compare_exchange_strong( none, first + k ); continue; }
        rebase_records( j.mbs, masks, dense, nmb, j.mbs_out, j.coeffs_out );
      }
    };
    const int workers = std::max( 1, std::min( worker_threads( 0 ), count ) );
    if ( workers == 1 ) work();
    else {
      std::vector<std::thread> pool;
      for ( int t = 0; t < workers; t++ ) pool.emplace_back( work );
      for ( auto & t : pool ) t.join();
    }
    ms_records += now_ms() - t_records;
    if ( short_job >= 0 ) {
      const int i = short_job;
      return no( AA_ERR_ARGUMENT, i, "coefficient buffer too small: " + std::to_string( jobs[i].num_coeff_blocks ) + " blocks needed, room for " + std::to_string( jobs[i].coeff_capacity_blocks ) );
    }
    first += count;
  }

  // ---- 6. the frames join their streams, as aa_stream_append_records appends them ----
  const double t_append = now_ms();
  // (a worker per stream at a time, as the host route of aa_submit_frames parses: the copy into a stream's pinned chunk is most of it)
  {
    std::vector<aa_status> status( n, AA_OK );
    std::vector<std::string> message( n );
    std::atomic<int> next { 0 };
    auto work = [&]() {
      (void) hipSetDevice( ctx->device );
      for ( ;; ) {
        const int i = next.fetch_add( 1 );
        if ( i >= n ) return;
        aa_rebase_job & j = jobs[i];
        aa_frame_header h = *j.hdr;
        h.key_frame = 0; h.num_coeff_blocks = j.num_coeff_blocks;
        h.num_intra_mbs = intra_mbs[i]; h.has_intra_mb = intra_mbs[i] != 0;
        status[i] = aa_stream_append_records( j.stream, &h, j.mbs_out, j.coeffs_out, &j.frame_index );
        if ( status[i] != AA_OK ) message[i] = g_last_error;
      }
    };
    const int workers = std::max( 1, std::min( worker_threads( 0 ), n ) );
    if ( workers == 1 ) work();
    else {
      std::vector<std::thread> pool;
      for ( int t = 0; t < workers; t++ ) pool.emplace_back( work );
      for ( auto & t : pool ) t.join();
    }
    for ( int i = 0; i < n; i++ ) if ( status[i] != AA_OK ) return fail( status[i], message[i] );
  }
  const double t_end = now_ms();
  const double timing[5] = { t_end - t_call, ms_kernels, ms_download, ms_records, t_end - t_append };
  std::memcpy( ctx->rebase_timing, timing, sizeof timing );
  return AA_OK;
}

aa_status aa_rebase_last_timing( aa_ctx * ctx, double out[5] )
{
  if ( !ctx || !out ) return fail( AA_ERR_ARGUMENT, "aa_rebase_last_timing: null argument" );
  std::memcpy( out, ctx->rebase_timing, sizeof ctx->rebase_timing );
  return AA_OK;
}

} // extern "C"
