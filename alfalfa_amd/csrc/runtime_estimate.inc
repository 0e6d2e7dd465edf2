// runtime.cpp (ABI): the frame-size estimate and the target-size quantiser search (aa_estimate_size_batch, aa_target_size_batch;
// Encoder::estimate_frame_size, size_estimation.cc, and Encoder::encode_with_target_size, encoder.cc:592-629).  An estimate is the forward
// encoder's first pass over every fourth macroblock of the picture in each direction as a small frame of its own, and that frame's
// serialised size times 16: the decisions and the DCT partition's byte count on the device (estimate_kernels.hip), the first partition
// from the small frame's records on the host (serializer.cpp: estimate_frame_bytes).  The search runs in rounds -- one estimate per
// unfinished job, the midpoint the reference would try -- with the rule of qi_choose.hh continued per job on the host between them.
// Nothing is appended, no DecoderState advances, no reference is touched.  The job table ring, the slice bound and the device pieces
// are the rebase's (runtime_rebase.inc).
namespace {

// One estimate of a round: a picture, a kind, a quality, a quantiser index and the carry in front of it -> its size and the carry behind it
struct EstimateItem {
  aa_stream * s;
  aa_quality_ref target;
  bool key;
  int quality, q_index;
  uint8_t carry[4];
  uint64_t size;
};

struct EstimateTiming { double decisions = 0, tokens = 0, download = 0, host = 0; int rounds = 0; };

uint32_t estimate_small_mbs( const aa_stream * s, uint32_t * mbw = nullptr, uint32_t * mbh = nullptr )
{
  const uint32_t w = ( s->parser.width() / 4u + 15u ) / 16u, h = ( s->parser.height() / 4u + 15u ) / 16u;
  if ( mbw ) *mbw = w;
  if ( mbh ) *mbh = h;
  return w * h;
}

// What both calls refuse of a job, in one order and one wording
template <class Job>
aa_status estimate_check_job( const char * who, aa_ctx * ctx, const Job * jobs, int i )
{
  const auto no = [who]( aa_status code, int k, const std::string & what ) { return fail( code, std::string( who ) + ": job " + std::to_string( k ) + ": " + what ); };
  const Job & j = jobs[i];
  if ( !j.stream || !j.target.y || !j.target.u || !j.target.v ) return no( AA_ERR_ARGUMENT, i, "null pointer" );
  aa_stream * s = j.stream;
  if ( s->ctx != ctx ) return no( AA_ERR_ARGUMENT, i, "stream belongs to another context" );
  for ( int k = 0; k < i; k++ ) if ( jobs[k].stream == s ) return no( AA_ERR_ARGUMENT, i, "its stream is also job " + std::to_string( k ) + "'s: one picture per stream and call" );
  if ( j.quality != AA_REENCODE_BEST && j.quality != AA_REENCODE_REALTIME ) return no( AA_ERR_ARGUMENT, i, "quality is neither AA_REENCODE_BEST nor AA_REENCODE_REALTIME" );
  if ( j.target.y_stride < int64_t( s->pw ) || j.target.uv_stride < int64_t( s->pw / 2 ) ) return no( AA_ERR_ARGUMENT, i, "row stride smaller than the padded plane's width" );
  if ( s->parser.width() < 4 || s->parser.height() < 4 )
    return no( AA_ERR_UNSUPPORTED, i, "a display width or height under 4: the estimate's frame of a quarter of the size would have no pixel" );
  if ( !j.key_frame ) {
    if ( s->next_submit != static_cast<int>( s->frames.size() ) ) return no( AA_ERR_LOGIC, i, "its stream holds a frame that is appended but not decoded: the references are not current" );
    if ( s->cur_ref_slot[0] < 0 || !s->slots[s->cur_ref_slot[0]].dev || s->slots[s->cur_ref_slot[0]].shared )
      return no( AA_ERR_LOGIC, i, "its stream's last reference is not a decoded or imported raster: an inter estimate needs a key frame before it" );
  }
  return AA_OK;
}

// One round: every item's estimate, slice by slice.  Per slice one upload (job table | size table | cost blocks | token tables), the
// decision kernels (key items first, each kind once), k_estimate_tokens, one download (three words | masks | records per item), then the
// first partitions on the host, one worker per item at a time.
aa_status estimate_round( aa_ctx * ctx, const std::string & who, std::vector<EstimateItem> & items, EstimateTiming & tm )
{
  const int n = static_cast<int>( items.size() );
  if ( !n ) return AA_OK;
  tm.rounds++;
  const size_t share = rebase_slice_bytes( ctx );
  for ( int first = 0; first < n; ) {
    int count = 0;
    size_t dense_total = 0, down_total = 0, side_total = 0, raster_total = 0, costs_total = 0;
    while ( first + count < n ) {
      const EstimateItem & it = items[first + count];
      const size_t nmb = estimate_small_mbs( it.s );
      if ( count && ( ctx->target_jobs_per_slice ? count >= ctx->target_jobs_per_slice : dense_total + nmb * AA_REBASE_MB_BYTES > share ) ) break;
      dense_total += align_up( nmb * AA_REBASE_MB_BYTES );
      down_total += align_up( 16 ) + align_up( nmb * sizeof( uint32_t ) ) + align_up( nmb * sizeof( aa_mb_info ) );
      side_total += align_up( nmb * sizeof( aa::ReencNeighbour ) ); raster_total += align_up( nmb * 384 );
      costs_total += align_up( it.key ? sizeof( aa::EstKeyCosts ) : sizeof( aa::EstInterCosts ) ) + align_up( 1056 );
      count++;
    }
    std::vector<int> at_item;                      // table entry -> item of the round: key items first, so that each kernel finds its kind in one run
    for ( int k = 0; k < count; k++ ) if ( items[first + k].key ) at_item.push_back( first + k );
    const int keys = static_cast<int>( at_item.size() );
    for ( int k = 0; k < count; k++ ) if ( !items[first + k].key ) at_item.push_back( first + k );

    const size_t table_bytes = align_up( size_t( count ) * sizeof( aa_reencode_dev_job ) ), sizes_bytes = align_up( size_t( count ) * sizeof( aa_estimate_dev_job ) );
    const size_t up_bytes = table_bytes + sizes_bytes + costs_total;
    const size_t piece_bytes = up_bytes + down_total + dense_total + side_total + raster_total;
    JobRing::Entry * rb = nullptr;
    if ( aa_status st = ctx->rebase_ring.take( up_bytes, align_up( 64 * sizeof( aa_rebase_dev_job ) ), &rb ) ) return st;
    uint8_t * piece = nullptr;
    if ( aa_status st = dev_alloc_compute( ctx, piece_bytes, &piece ) ) return st;
    struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { dev_free_compute( c, p, b ); } } back { ctx, piece, piece_bytes };
    size_t staging_bytes = 0;
    uint8_t * staging = pinned_get( ctx, down_total, &staging_bytes );
    if ( !staging ) return fail( AA_ERR_HIP, who + ": pinned staging allocation failed" );
    struct Unpin { aa_ctx * c; uint8_t * p; size_t b; ~Unpin() { std::lock_guard<std::mutex> g( c->pool_mu ); c->pinned_pool.emplace_back( p, b ); } } unpin { ctx, staging, staging_bytes };

    aa_reencode_dev_job * table = reinterpret_cast<aa_reencode_dev_job *>( rb->host );
    aa_estimate_dev_job * sizes = reinterpret_cast<aa_estimate_dev_job *>( rb->host + table_bytes );
    std::vector<size_t> down_off( count );
    std::vector<std::vector<uint8_t>> probs_before( count );
    size_t up_off = table_bytes + sizes_bytes, dn_off = 0, rest_off = up_bytes + down_total;
    for ( int k = 0; k < count; k++ ) {
      const EstimateItem & it = items[at_item[k]];
      aa_stream * s = it.s;
      uint32_t mbw = 0, mbh = 0;
      const size_t nmb = estimate_small_mbs( s, &mbw, &mbh );
      aa_reencode_dev_job & d = table[k];
      std::memset( &d, 0, sizeof d );
      if ( !it.key ) for ( int p = 0; p < 3; p++ ) d.base.ref[1][p] = slot_plane( s, s->cur_ref_slot[0], p );
      d.base.target[0] = static_cast<const uint8_t *>( it.target.y ); d.base.target[1] = static_cast<const uint8_t *>( it.target.u ); d.base.target[2] = static_cast<const uint8_t *>( it.target.v );
      d.base.target_stride[0] = it.target.y_stride; d.base.target_stride[1] = it.target.uv_stride;
      uint16_t quant[6];
      const int no_delta[5] = { 0, 0, 0, 0, 0 };
      aa::quant_factors( it.q_index, no_delta, quant );                  // QuantIndices with y_ac_qi alone (size_estimation.cc:49-50,111-112)
      std::memcpy( d.base.quant, quant, sizeof d.base.quant );
      d.base.mbw = static_cast<uint16_t>( mbw ); d.base.mbh = static_cast<uint16_t>( mbh ); d.base.has_intra = 1;
      // the cost block: the forward encoder's, the original's size behind it; an inter estimate in front of the encoder's first inter
      // frame meets vector cost tables that are still all zero (carry[3] == 0; size_estimation.cc never fills them)
      d.costs = piece + up_off;
      probs_before[k].assign( 1101, 0 );
      if ( it.key ) {
        aa::EstKeyCosts & C = *reinterpret_cast<aa::EstKeyCosts *>( rb->host + up_off );
        aa::enc_fill_key_costs( C.enc, quant[1] );
        C.full_mbw = s->parser.mb_width(); C.full_mbh = s->parser.mb_height();
        up_off += align_up( sizeof C );
        aa::ProbTables defaults;
        defaults.set_defaults();
        std::memcpy( rb->host + up_off, &defaults.coeff[0][0][0][0], 1056 );
      } else {
        aa::EstInterCosts & C = *reinterpret_cast<aa::EstInterCosts *>( rb->host + up_off );
        aa::enc_fill_inter_costs( C.enc, s->parser.probs().mv, it.quality, quant[1], static_cast<unsigned>( it.q_index ) );
        if ( !it.carry[3] ) { std::memset( C.enc.base.mv_comp, 0, sizeof C.enc.base.mv_comp ); std::memset( C.enc.mv_sad, 0, sizeof C.enc.mv_sad ); }
        C.full_mbw = s->parser.mb_width(); C.full_mbh = s->parser.mb_height();
        up_off += align_up( sizeof C );
        export_probs( s->parser, probs_before[k].data() );
        std::memcpy( rb->host + up_off, probs_before[k].data(), 1056 );
      }
      sizes[k].token_probs = piece + up_off;
      up_off += align_up( 1056 );
      down_off[k] = dn_off;
      sizes[k].result = reinterpret_cast<uint32_t *>( piece + up_bytes + dn_off ); dn_off += align_up( 16 );
      d.base.masks = reinterpret_cast<uint32_t *>( piece + up_bytes + dn_off ); dn_off += align_up( nmb * sizeof( uint32_t ) );
      d.mbs_out = reinterpret_cast<aa_mb_info *>( piece + up_bytes + dn_off ); dn_off += align_up( nmb * sizeof( aa_mb_info ) );
      d.base.coeffs = reinterpret_cast<int16_t *>( piece + rest_off ); rest_off += align_up( nmb * AA_REBASE_MB_BYTES );
      d.nb = reinterpret_cast<uint32_t *>( piece + rest_off ); rest_off += align_up( nmb * sizeof( aa::ReencNeighbour ) );
      // the reconstruction of the small frame: planes of ITS padded size (the reference's raster is the original's size with this corner written)
      d.base.recon[0] = piece + rest_off; d.base.recon[1] = piece + rest_off + nmb * 256; d.base.recon[2] = piece + rest_off + nmb * 320;
      rest_off += align_up( nmb * 384 );
    }
    hipEvent_t ev[4] = { get_event( ctx ), get_event( ctx ), get_event( ctx ), get_event( ctx ) };
    struct Events { aa_ctx * c; hipEvent_t * e; ~Events() { for ( int i = 0; i < 4; i++ ) if ( e[i] ) c->free_events.push_back( e[i] ); } } events { ctx, ev };
    if ( !ev[0] || !ev[1] || !ev[2] || !ev[3] ) return fail( AA_ERR_HIP, who + ": hipEventCreate failed" );
    const aa_reencode_dev_job * dev_table = reinterpret_cast<const aa_reencode_dev_job *>( piece );
    const aa_estimate_dev_job * dev_sizes = reinterpret_cast<const aa_estimate_dev_job *>( piece + table_bytes );
    HIP_TRY( hipEventRecord( ev[0], ctx->compute ) );
    HIP_TRY( hipMemcpyAsync( piece, rb->host, up_bytes, hipMemcpyHostToDevice, ctx->compute ) );
    if ( aa_status st = ctx->rebase_ring.mark( *rb, ctx->compute ) ) return st;
    if ( keys ) if ( int e = aa::launch_estimate( dev_table, keys, true, ctx->reenc_slots, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_estimate_key" );
    if ( count > keys ) if ( int e = aa::launch_estimate( dev_table + keys, count - keys, false, ctx->reenc_slots, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_estimate_inter" );
    HIP_TRY( hipEventRecord( ev[1], ctx->compute ) );
    // a lane is one chain of dependent instructions: spread the jobs over the chip's SIMDs before any wave gets a second one
    const int simds = ctx->tok.n_cus > 0 ? ctx->tok.n_cus * 4 : 1024;
    const int lanes_per_wave = std::max( 1, std::min( 64, ( count + simds - 1 ) / simds ) );
    if ( int e = aa::launch_estimate_tokens( dev_table, dev_sizes, count, lanes_per_wave, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_estimate_tokens" );
    HIP_TRY( hipEventRecord( ev[2], ctx->compute ) );
    HIP_TRY( hipMemcpyAsync( staging, piece + up_bytes, down_total, hipMemcpyDeviceToHost, ctx->compute ) );
    HIP_TRY( hipEventRecord( ev[3], ctx->compute ) );
    HIP_TRY( hipStreamSynchronize( ctx->compute ) );
    if ( aa_status st = check_watchdog( ctx ) ) return st;
    { float a = 0, b = 0, c = 0;
      if ( hipEventElapsedTime( &a, ev[0], ev[1] ) == hipSuccess && hipEventElapsedTime( &b, ev[1], ev[2] ) == hipSuccess && hipEventElapsedTime( &c, ev[2], ev[3] ) == hipSuccess ) {
        tm.decisions += a; tm.tokens += b; tm.download += c; } }

    // the sizes: header and first partition on the host, one worker per item at a time
    const double t_host = now_ms();
    std::atomic<int> next { 0 }, failed { -1 };
    std::vector<std::string> message( count );
    auto work = [&]() {
      for ( ;; ) {
        const int k = next.fetch_add( 1 );
        if ( k >= count ) return;
        EstimateItem & it = items[at_item[k]];
        const size_t nmb = estimate_small_mbs( it.s );
        const uint8_t * at = staging + down_off[k];
        const uint32_t * words = reinterpret_cast<const uint32_t *>( at ); at += align_up( 16 );
        const uint32_t * masks = reinterpret_cast<const uint32_t *>( at ); at += align_up( nmb * sizeof( uint32_t ) );
        const aa_mb_info * recs = reinterpret_cast<const aa_mb_info *>( at );
        try {
          const size_t bytes = aa::estimate_frame_bytes( it.key, static_cast<uint16_t>( it.s->parser.width() / 4 ), static_cast<uint16_t>( it.s->parser.height() / 4 ),
                                                         static_cast<uint8_t>( it.q_index ), it.key ? nullptr : probs_before[k].data(), recs, masks, words[0], words[1], words[2], it.carry );
          it.size = uint64_t( bytes ) * 16;         // WIDTH_SAMPLE_DIMENSION_FACTOR * HEIGHT_SAMPLE_DIMENSION_FACTOR
        } catch ( const aa::ParseError & e ) {
          message[k] = e.message;
          int none = -1; failed.compare_exchange_strong( none, k );
        }
      }
    };
    const int workers = std::max( 1, std::min( worker_threads( 0 ), count ) );
    if ( workers == 1 ) work();
    else {
      std::vector<std::thread> pool;
      for ( int t = 0; t < workers; t++ ) pool.emplace_back( work );
      for ( auto & t : pool ) t.join();
    }
    tm.host += now_ms() - t_host;
    if ( failed >= 0 ) return fail( AA_ERR_LOGIC, who + ": job " + std::to_string( at_item[failed] ) + ": " + message[failed] );
    first += count;
  }
  return AA_OK;
}

void estimate_store_timing( aa_ctx * ctx, double t_call, const EstimateTiming & tm )
{
  const double timing[6] = { now_ms() - t_call, tm.decisions, tm.tokens, tm.download, tm.host, double( tm.rounds ) };
  std::memcpy( ctx->target_size_timing, timing, sizeof timing );
}

} // namespace

extern "C" {

void aa_target_size_range( int last_q, int * q_lo, int * q_hi )
{
  int lo, hi;
  aa::qi_target_range( last_q, lo, hi );
  if ( q_lo ) *q_lo = lo;
  if ( q_hi ) *q_hi = hi;
}

aa_status aa_ctx_set_target_size_round( aa_ctx * ctx, int jobs_per_slice )
{
  if ( !ctx || jobs_per_slice < 0 ) return fail( AA_ERR_ARGUMENT, "aa_ctx_set_target_size_round: jobs per slice: 0 (by memory) or more" );
  ctx->target_jobs_per_slice = jobs_per_slice;
  return AA_OK;
}

aa_status aa_target_size_last_timing( aa_ctx * ctx, double out[6] )
{
  if ( !ctx || !out ) return fail( AA_ERR_ARGUMENT, "aa_target_size_last_timing: null argument" );
  std::memcpy( out, ctx->target_size_timing, sizeof ctx->target_size_timing );
  return AA_OK;
}

aa_status aa_estimate_size_batch( aa_ctx * ctx, aa_estimate_size_job * jobs, int n )
{
  const std::string who = "aa_estimate_size_batch";
  if ( !ctx || n < 0 || ( n && !jobs ) ) return fail( AA_ERR_ARGUMENT, who + ": bad argument" );
  if ( !n ) return AA_OK;
  if ( aa_status st = set_device( ctx ) ) return st;
  for ( int i = 0; i < n; i++ ) {
    if ( aa_status st = estimate_check_job( who.c_str(), ctx, jobs, i ) ) return st;
    if ( jobs[i].q_index < 0 || jobs[i].q_index > 127 ) return fail( AA_ERR_ARGUMENT, who + ": job " + std::to_string( i ) + ": q_index outside 0..127" );
  }
  const double t_call = now_ms();
  std::vector<EstimateItem> items( n );
  for ( int i = 0; i < n; i++ ) {
    const aa_estimate_size_job & j = jobs[i];
    EstimateItem & it = items[i];
    it.s = j.stream; it.target = j.target; it.key = j.key_frame != 0; it.quality = j.quality; it.q_index = j.q_index; it.size = 0;
    std::memcpy( it.carry, j.carry, 4 );
  }
  EstimateTiming tm;
  if ( aa_status st = estimate_round( ctx, who, items, tm ) ) return st;
  for ( int i = 0; i < n; i++ ) {
    jobs[i].size_out = items[i].size;
    if ( !items[i].key ) std::memcpy( jobs[i].carry, items[i].carry, 3 );
  }
  estimate_store_timing( ctx, t_call, tm );
  return AA_OK;
}

aa_status aa_target_size_batch( aa_ctx * ctx, aa_target_size_job * jobs, int n )
{
  const std::string who = "aa_target_size_batch";
  if ( !ctx || n < 0 || ( n && !jobs ) ) return fail( AA_ERR_ARGUMENT, who + ": bad argument" );
  if ( !n ) return AA_OK;
  if ( aa_status st = set_device( ctx ) ) return st;
  for ( int i = 0; i < n; i++ ) {
    if ( aa_status st = estimate_check_job( who.c_str(), ctx, jobs, i ) ) return st;
    const aa_target_size_job & j = jobs[i];
    if ( j.q_lo < 0 || j.q_lo > 127 || j.q_hi < 0 || j.q_hi > 127 ) return fail( AA_ERR_ARGUMENT, who + ": job " + std::to_string( i ) + ": q_lo or q_hi outside 0..127" );
    if ( j.q_lo > j.q_hi ) return fail( AA_ERR_ARGUMENT, who + ": job " + std::to_string( i ) + ": q_lo > q_hi" );
  }
  const double t_call = now_ms();
  // every job's search between rounds, what it has visited, and the carry that runs through its estimates
  struct Search { aa::QiChoice c; uint8_t carry[4]; int visited_q[aa::kQiMaxSteps]; uint64_t visited_size[aa::kQiMaxSteps]; };
  std::vector<Search> searches( n );
  for ( int i = 0; i < n; i++ ) { aa::qi_choice_begin( searches[i].c, jobs[i].q_lo, jobs[i].q_hi ); std::memcpy( searches[i].carry, jobs[i].carry, 4 ); }
  EstimateTiming tm;
  for ( ;; ) {
    std::vector<EstimateItem> items;
    std::vector<int> job_of;
    for ( int i = 0; i < n; i++ ) {
      Search & sr = searches[i];
      if ( aa::qi_choice_done( sr.c ) ) continue;
      if ( sr.c.steps >= aa::kQiMaxSteps ) return fail( AA_ERR_LOGIC, who + ": job " + std::to_string( i ) + ": the search did not end within " + std::to_string( aa::kQiMaxSteps ) + " estimates" );
      EstimateItem it;
      it.s = jobs[i].stream; it.target = jobs[i].target; it.key = jobs[i].key_frame != 0; it.quality = jobs[i].quality;
      it.q_index = aa::qi_choice_candidate( sr.c ); it.size = 0;
      std::memcpy( it.carry, sr.carry, 4 );
      items.push_back( it ); job_of.push_back( i );
    }
    if ( items.empty() ) break;
    if ( aa_status st = estimate_round( ctx, who, items, tm ) ) return st;
    const double t_rule = now_ms();
    for ( size_t k = 0; k < items.size(); k++ ) {
      Search & sr = searches[job_of[k]];
      sr.visited_q[sr.c.steps] = items[k].q_index; sr.visited_size[sr.c.steps] = items[k].size;
      if ( !items[k].key ) std::memcpy( sr.carry, items[k].carry, 3 );
      aa::qi_choice_step( sr.c, items[k].size, jobs[job_of[k]].target_size );
    }
    tm.host += now_ms() - t_rule;
  }
  for ( int i = 0; i < n; i++ ) {
    const Search & sr = searches[i];
    aa_target_size_job & j = jobs[i];
    j.q_index = sr.c.best; j.estimates = sr.c.steps;
    for ( int k = 0; k < aa::kQiMaxSteps; k++ ) { j.visited_q[k] = k < sr.c.steps ? sr.visited_q[k] : 0; j.visited_size[k] = k < sr.c.steps ? sr.visited_size[k] : 0; }
    std::memcpy( j.carry, sr.carry, 3 );
  }
  estimate_store_timing( ctx, t_call, tm );
  return AA_OK;
}

} // extern "C"
