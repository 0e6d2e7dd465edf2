// runtime.cpp (ABI), its last piece: the rebase (aa_rebase_batch) -- inter frames' residues recomputed against the job streams' current
// references on the device, the records built on the host and appended as aa_stream_append_records appends them; kernels in
// rebase_kernels.hip -- or (aa_rebase_device_batch) compacted on the device into a piece of HBM that is the frame's from then on; kernels
// in rebase_compact_kernels.hip, the rule in rebase_compact.hh.  And aa_quant_factors, the quantiser of a new frame's header.
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

// Job i of a rebase call (aa_rebase_job or aa_rebase_device_job: stream, hdr, mbs, target) against the jobs before it: what both entry
// points refuse, in one order and one wording.  `who`: the ABI call, in front of the message.
template <class Job>
aa_status rebase_check_job( const char * who, aa_ctx * ctx, const Job * jobs, int i )
{
  const auto no = [who]( aa_status code, int k, const std::string & what ) { return fail( code, std::string( who ) + ": job " + std::to_string( k ) + ": " + what ); };
  const Job & j = jobs[i];
  if ( !j.stream || !j.hdr || !j.mbs || !j.target.y || !j.target.u || !j.target.v ) return no( AA_ERR_ARGUMENT, i, "null pointer" );
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
  return AA_OK;
}

// What a slice's kernels read of one job, into its entry of the job table: references, target, quantiser, and where its input records,
// masks, dense slots and reconstruction lie in the slice's piece (has_intra is the caller's: it reads the records anyway).
template <class Job>
void rebase_fill_job( aa_rebase_dev_job & d, const Job & j, uint8_t * records, uint8_t * masks, uint8_t * dense, uint8_t * raster )
{
  aa_stream * s = j.stream;
  std::memset( &d, 0, sizeof d );
  for ( int r = 0; r < 3; r++ ) for ( int p = 0; p < 3; p++ ) d.ref[1 + r][p] = slot_plane( s, s->cur_ref_slot[r], p );
  d.target[0] = static_cast<const uint8_t *>( j.target.y ); d.target[1] = static_cast<const uint8_t *>( j.target.u ); d.target[2] = static_cast<const uint8_t *>( j.target.v );
  d.target_stride[0] = j.target.y_stride; d.target_stride[1] = j.target.uv_stride;
  d.recon[0] = raster; d.recon[1] = raster + s->plane_bytes[0]; d.recon[2] = raster + s->plane_bytes[0] + s->plane_bytes[1];
  d.mbs = reinterpret_cast<const aa_mb_info *>( records );
  d.masks = reinterpret_cast<uint32_t *>( masks );
  d.coeffs = reinterpret_cast<int16_t *>( dense );
  std::memcpy( d.quant, j.hdr->quant[0], sizeof d.quant );
  d.mbw = j.hdr->mb_width; d.mbh = j.hdr->mb_height;
}

// A device-resident frame's piece comes in few sizes: beyond 64 KiB a sixteenth of the next power of two (at most 6 % over), as the pool
// rounds its big pieces -- the pool keeps freed pieces in per-size lists and does not re-split them, and a piece per block count would
// leave a list per block count behind.
size_t rebase_piece_bytes( size_t exact )
{
  exact = align_up( exact );
  if ( exact <= ( size_t( 64 ) << 10 ) ) return exact;
  size_t p2 = size_t( 64 ) << 10;
  while ( p2 < exact ) p2 <<= 1;
  const size_t step = p2 / 16;
  return ( exact + step - 1 ) / step * step;
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
    if ( !j.mbs_out || ( !j.coeffs_out && j.coeff_capacity_blocks ) ) return no( AA_ERR_ARGUMENT, i, "null pointer" );
    if ( aa_status st = rebase_check_job( "aa_rebase_batch", ctx, jobs, i ) ) return st;
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
      rebase_fill_job( d, j, piece + up_off, piece + up_bytes + res_off, piece + up_bytes + res_off + align_up( nmb * sizeof( uint32_t ) ), piece + raster_off );
      raster_off += s->slot_bytes;
      std::memcpy( rb->host + up_off, j.mbs, nmb * sizeof( aa_mb_info ) );
      up_off += align_up( nmb * sizeof( aa_mb_info ) );
      result_off[k] = res_off;
      res_off += align_up( nmb * sizeof( uint32_t ) ) + align_up( nmb * AA_REBASE_MB_BYTES );
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

/* The rebase with the new frame's records kept in HBM: the kernels of aa_rebase_batch, then k_rebase_count / k_rebase_compact
 * (rebase_compact_kernels.hip) in place of the download, rebase_records and the append.  Per slice one small copy comes down -- the
 * blocks stored per run of 256 macroblocks -- and the host sums it into the frames' block counts, allocates every frame's piece at that
 * size and hands the pieces to the second kernel.  A frame's FrameRec is a host-appended frame's without the host half: no chunk, no
 * batch, rec_block = the piece (job record | macroblock records | intra-row words | dense blocks), dev_job = its start. */
aa_status aa_rebase_device_batch( aa_ctx * ctx, aa_rebase_device_job * jobs, int n )
{
  if ( !ctx || !jobs || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_rebase_device_batch: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  // ---- 1. the arguments: nothing is launched, nothing appended unless every job of the call is good ----
  for ( int i = 0; i < n; i++ ) {
    if ( aa_status st = rebase_check_job( "aa_rebase_device_batch", ctx, jobs, i ) ) return st;
    jobs[i].num_coeff_blocks = 0; jobs[i].num_intra_mbs = 0; jobs[i].frame_index = -1;
  }

  const double t_call = now_ms();
  // the frames in the making: what the host knows of them from the input records (the rebase keeps every mode and reference) and their
  // pieces, which go back to the pool unless the whole call succeeds (through an epoch: k_rebase_compact may be queued on them)
  struct Made { FrameRec rec; uint8_t * piece = nullptr; size_t bytes = 0; };
  std::vector<Made> made( n );
  struct GiveBack { aa_ctx * c; std::vector<Made> & m; bool keep = false;
                    ~GiveBack() { if ( !keep ) for ( Made & x : m ) dev_free( c, x.piece, x.bytes, true ); } } give_back { ctx, made };
  std::vector<hipEvent_t> events;            // five per slice: [0..1] table up, rebase, count; [1..2] partial sums down; [3..4] second table up, compaction
  struct Events { aa_ctx * c; std::vector<hipEvent_t> & e; ~Events() { for ( hipEvent_t x : e ) if ( x ) c->free_events.push_back( x ); } } events_back { ctx, events };

  // ---- 2..5. slice by slice: job table and records up, the rebase kernels and the count, the partial sums down, pieces, the compaction ----
  const size_t share = rebase_slice_bytes( ctx );
  const size_t job_bytes = align_up( sizeof( aa_dev_frame ) );
  for ( int first = 0; first < n; ) {
    int count = 0;
    size_t dense_total = 0, masks_total = 0, records_total = 0, raster_total = 0, rows_total = 0;
    uint32_t max_mbs = 0;
    while ( first + count < n ) {
      const aa_stream * s = jobs[first + count].stream;
      const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
      if ( count && dense_total + nmb * AA_REBASE_MB_BYTES > share ) break;
      dense_total += align_up( nmb * AA_REBASE_MB_BYTES ); masks_total += align_up( nmb * sizeof( uint32_t ) );
      records_total += align_up( nmb * sizeof( aa_mb_info ) );
      rows_total += align_up( size_t( ( s->parser.mb_width() + 63 ) / 64 ) * s->parser.mb_height() * sizeof( unsigned long long ) );
      raster_total += s->slot_bytes;
      max_mbs = std::max<uint32_t>( max_mbs, static_cast<uint32_t>( nmb ) );
      count++;
    }
    // the slice's piece: job table | input records (one upload) | compaction table | intra-row words (a second one, once the pieces are
    // known) | partial sums | masks | dense slots | reconstruction rasters.  Pinned: a JobRing entry for each upload; the partial sums
    // come down behind the first one's table.
    const uint32_t stride = aa::compact::runs_of( max_mbs );
    const size_t table_bytes = align_up( size_t( count ) * sizeof( aa_rebase_dev_job ) );
    const size_t up_bytes = table_bytes + records_total;
    const size_t ctable_bytes = align_up( size_t( count ) * sizeof( aa_rebase_compact_job ) );
    const size_t up2_bytes = ctable_bytes + rows_total;
    const size_t partial_bytes = align_up( size_t( count ) * stride * sizeof( uint32_t ) );
    const size_t result_bytes = masks_total + dense_total;
    const size_t piece_bytes = up_bytes + up2_bytes + partial_bytes + result_bytes + raster_total;
    JobRing::Entry * rb = nullptr, * rb2 = nullptr;
    if ( aa_status st = ctx->rebase_ring.take( up_bytes + partial_bytes, align_up( 64 * sizeof( aa_rebase_dev_job ) ), &rb ) ) return st;
    if ( aa_status st = ctx->rebase_ring.take( up2_bytes, align_up( 64 * sizeof( aa_rebase_compact_job ) ), &rb2 ) ) return st;
    uint8_t * piece = nullptr;
    if ( aa_status st = dev_alloc_compute( ctx, piece_bytes, &piece ) ) return st;
    struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { dev_free_compute( c, p, b ); } } back { ctx, piece, piece_bytes };
    uint8_t * const piece2 = piece + up_bytes;
    uint32_t * const partials_dev = reinterpret_cast<uint32_t *>( piece2 + up2_bytes );
    uint8_t * const results = piece2 + up2_bytes + partial_bytes;

    aa_rebase_dev_job * table = reinterpret_cast<aa_rebase_dev_job *>( rb->host );
    aa_rebase_compact_job * ctable = reinterpret_cast<aa_rebase_compact_job *>( rb2->host );
    size_t up_off = table_bytes, rows_off = ctable_bytes, res_off = 0, raster_off = up_bytes + up2_bytes + partial_bytes + result_bytes;
    bool any_intra = false;
    for ( int k = 0; k < count; k++ ) {
      aa_rebase_device_job & j = jobs[first + k];
      aa_stream * s = j.stream;
      const int mbw = j.hdr->mb_width, mbh = j.hdr->mb_height;
      const size_t nmb = size_t( mbw ) * mbh;
      aa_rebase_dev_job & d = table[k];
      rebase_fill_job( d, j, piece + up_off, results + res_off, results + res_off + align_up( nmb * sizeof( uint32_t ) ), piece + raster_off );
      raster_off += s->slot_bytes;
      std::memcpy( rb->host + up_off, j.mbs, nmb * sizeof( aa_mb_info ) );
      up_off += align_up( nmb * sizeof( aa_mb_info ) );
      res_off += align_up( nmb * sizeof( uint32_t ) ) + align_up( nmb * AA_REBASE_MB_BYTES );
      // what append_host_frame reads off a frame's records: intra macroblocks by row and by 2:1 anti-diagonal, SPLITMV
      FrameRec & rec = made[first + k].rec;
      const size_t words_per_row = ( mbw + 63 ) / 64;
      unsigned long long * rows = reinterpret_cast<unsigned long long *>( rb2->host + rows_off );
      std::memset( rows, 0, words_per_row * mbh * sizeof( unsigned long long ) );
      rec.intra_diagonals.assign( mbw + 2 * ( mbh - 1 ), 0 );
      uint32_t intra = 0;
      for ( int r = 0; r < mbh; r++ ) for ( int col = 0; col < mbw; col++ ) {
        const aa_mb_info & mb = j.mbs[size_t( r ) * mbw + col];
        if ( mb.ref_frame == 0 ) { intra++; rec.intra_diagonals[col + 2 * r] = 1; rows[r * words_per_row + ( col >> 6 )] |= 1ull << ( col & 63 ); }
        else if ( mb.y_mode == 9 /* SPLITMV */ ) rec.has_split = true;
      }
      j.num_intra_mbs = intra;
      d.has_intra = intra != 0;
      any_intra = any_intra || d.has_intra;
      aa_rebase_compact_job & o = ctable[k];
      std::memset( &o, 0, sizeof o );
      o.rows = reinterpret_cast<const unsigned long long *>( piece2 + rows_off );
      o.rows_words = static_cast<uint32_t>( words_per_row * mbh );
      rows_off += align_up( words_per_row * mbh * sizeof( unsigned long long ) );
    }
    hipEvent_t ev[5] = { get_event( ctx ), get_event( ctx ), get_event( ctx ), get_event( ctx ), get_event( ctx ) };
    events.insert( events.end(), ev, ev + 5 );
    if ( !ev[0] || !ev[1] || !ev[2] || !ev[3] || !ev[4] ) return fail( AA_ERR_HIP, "aa_rebase_device_batch: hipEventCreate failed" );
    HIP_TRY( hipEventRecord( ev[0], ctx->compute ) );
    HIP_TRY( hipMemcpyAsync( piece, rb->host, up_bytes, hipMemcpyHostToDevice, ctx->compute ) );
    if ( int e = aa::launch_rebase( reinterpret_cast<const aa_rebase_dev_job *>( piece ), count, max_mbs, any_intra, ctx->compute ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_rebase_inter / k_rebase_intra" );
    if ( int e = aa::launch_rebase_count( reinterpret_cast<const aa_rebase_dev_job *>( piece ), count, max_mbs, partials_dev, stride, ctx->compute ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_rebase_count" );
    HIP_TRY( hipEventRecord( ev[1], ctx->compute ) );
    uint32_t * const partials = reinterpret_cast<uint32_t *>( rb->host + up_bytes );
    HIP_TRY( hipMemcpyAsync( partials, partials_dev, size_t( count ) * stride * sizeof( uint32_t ), hipMemcpyDeviceToHost, ctx->compute ) );
    HIP_TRY( hipEventRecord( ev[2], ctx->compute ) );
    if ( aa_status st = ctx->rebase_ring.mark( *rb, ctx->compute ) ) return st;
    HIP_TRY( hipStreamSynchronize( ctx->compute ) );
    if ( aa_status st = check_watchdog( ctx ) ) return st;

    // every frame's block count, its piece at that size, and where the second kernel puts what
    for ( int k = 0; k < count; k++ ) {
      aa_rebase_device_job & j = jobs[first + k];
      Made & m = made[first + k];
      const size_t nmb = size_t( j.hdr->mb_width ) * j.hdr->mb_height;
      uint32_t blocks = 0;
      for ( uint32_t r = 0; r < aa::compact::runs_of( static_cast<uint32_t>( nmb ) ); r++ ) blocks += partials[size_t( k ) * stride + r];
      if ( blocks > nmb * 25 ) return fail( AA_ERR_HIP, "aa_rebase_device_batch: job " + std::to_string( first + k ) + ": k_rebase_count reports more blocks than the frame can hold" );
      j.num_coeff_blocks = blocks;
      const size_t mb_bytes = align_up( nmb * sizeof( aa_mb_info ) );
      const size_t rows_bytes = align_up( size_t( ctable[k].rows_words ) * sizeof( unsigned long long ) );
      m.bytes = rebase_piece_bytes( job_bytes + mb_bytes + rows_bytes + align_up( size_t( blocks ) * 32 ) );
      if ( aa_status st = dev_alloc( ctx, m.bytes, &m.piece ) ) return st;
      FrameRec & rec = m.rec;
      rec.hdr = *j.hdr;
      rec.hdr.key_frame = 0; rec.hdr.num_coeff_blocks = blocks;
      rec.hdr.num_intra_mbs = j.num_intra_mbs; rec.hdr.has_intra_mb = j.num_intra_mbs != 0;
      rec.rec_block = m.piece; rec.rec_bytes = m.bytes;
      rec.dev_job = reinterpret_cast<const aa_dev_frame *>( m.piece );
      rec.dev_mbs = reinterpret_cast<aa_mb_info *>( m.piece + job_bytes );
      aa_rebase_compact_job & o = ctable[k];
      fill_job( rec, &o.frame );
      o.out_frame = reinterpret_cast<aa_dev_frame *>( m.piece );
      o.out_mbs = rec.dev_mbs;
      o.out_rows = reinterpret_cast<unsigned long long *>( m.piece + job_bytes + mb_bytes );
      o.out_coeffs = reinterpret_cast<int16_t *>( m.piece + job_bytes + mb_bytes + rows_bytes );
      o.num_coeff_blocks = blocks;
      o.frame.mbs = o.out_mbs; o.frame.intra_rows = o.out_rows; o.frame.coeffs = o.out_coeffs;
    }
    HIP_TRY( hipEventRecord( ev[3], ctx->compute ) );
    HIP_TRY( hipMemcpyAsync( piece2, rb2->host, up2_bytes, hipMemcpyHostToDevice, ctx->compute ) );
    if ( int e = aa::launch_rebase_compact( reinterpret_cast<const aa_rebase_dev_job *>( piece ), reinterpret_cast<const aa_rebase_compact_job *>( piece2 ), count, max_mbs,
                                            partials_dev, stride, ctx->compute ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_rebase_compact" );
    HIP_TRY( hipEventRecord( ev[4], ctx->compute ) );
    if ( aa_status st = ctx->rebase_ring.mark( *rb2, ctx->compute ) ) return st;
    first += count;
  }
  // the call is synchronous, as aa_rebase_batch is: whoever reads the pieces next (a copy of another call, on no stream of this context's)
  // finds them written
  HIP_TRY( hipStreamSynchronize( ctx->compute ) );
  if ( aa_status st = check_watchdog( ctx ) ) return st;
  double ms_kernels = 0, ms_download = 0;
  for ( size_t e = 0; e + 4 < events.size(); e += 5 ) {
    float a = 0, b = 0, c = 0;
    if ( hipEventElapsedTime( &a, events[e], events[e + 1] ) == hipSuccess && hipEventElapsedTime( &b, events[e + 1], events[e + 2] ) == hipSuccess
         && hipEventElapsedTime( &c, events[e + 3], events[e + 4] ) == hipSuccess ) { ms_kernels += a + c; ms_download += b; }
  }

  // ---- 6. the frames join their streams: bookkeeping only ----
  const double t_append = now_ms();
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = jobs[i].stream;
    jobs[i].frame_index = static_cast<int>( s->frames.size() );
    s->frames.push_back( std::move( made[i].rec ) );
  }
  give_back.keep = true;
  const double t_end = now_ms();
  const double timing[5] = { t_end - t_call, ms_kernels, ms_download, 0.0, t_end - t_append };
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
