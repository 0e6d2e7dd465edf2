// runtime.cpp (ABI): the re-encode (aa_reencode_batch) -- a chunk's key frame encoded again as an inter frame predicted from the job
// streams' current references: the reference's mode decision and the forward path on the device (reencode_kernels.hip), the records
// built on the host and appended as aa_stream_append_records appends them -- or (aa_reencode_device_batch) compacted on the device into a
// piece of HBM that is the frame's from then on; kernels in reencode_compact_kernels.hip, the rule in reencode_compact.hh.  Modelled on
// aa_rebase_batch / aa_rebase_device_batch (runtime_rebase.inc), whose job-table ring, slice bound, piece sizes and record builder it shares.
// Both entry points are templates over their caller: the re-encode here, the forward encoder in runtime_encode.inc (aa_encode_batch /
// aa_encode_device_batch), whose jobs may be key frames and whose kernels are k_encode_key / k_encode_inter.
namespace {

// The re-encode as a caller of reencode_batch / reencode_device_batch.  kForward: jobs may be key frames, inter jobs need a decoded last
// reference, the cost blocks are the forward policies' (reencode_search.hh), and each kind has its own kernel.
struct ReencodeCall {
  static constexpr bool kForward = false;
  static constexpr const char * kHost = "aa_reencode_batch", * kDevice = "aa_reencode_device_batch";
  static double * timing( aa_ctx * ctx ) { return ctx->reencode_timing; }
};

// What the kernel left of a job -> the caller's records: flags, nz_mask and coeff_index by rebase_records, as the parser sets them for
// the serialised frame; lf_level from the new header (mb_lf_level) with the stream's current filter adjustments; segment_id 0.
RebaseCounts reencode_records( const aa_mb_info * in, const uint32_t * masks, const int16_t * dense, size_t nmb, const aa::HeaderParams & fp, aa_mb_info * out, int16_t * coeffs_out )
{
  const RebaseCounts c = rebase_records( in, masks, dense, nmb, out, coeffs_out );
  if ( out ) for ( size_t i = 0; i < nmb; i++ ) out[i].lf_level = aa::mb_lf_level( fp, 0, out[i].ref_frame, out[i].y_mode );
  return c;
}

// Job i of a re-encode call (aa_reencode_job or aa_reencode_device_job: stream, hdr, target, quality) against the jobs before it: what
// both entry points refuse, in one order and one wording.  `who`: the ABI call, in front of the message.
template <class Call, class Job>
aa_status reencode_check_job( const char * who, aa_ctx * ctx, const Job * jobs, int i )
{
  const auto no = [who]( aa_status code, int k, const std::string & what ) { return fail( code, std::string( who ) + ": job " + std::to_string( k ) + ": " + what ); };
  const Job & j = jobs[i];
  if ( !j.stream || !j.hdr || !j.target.y || !j.target.u || !j.target.v ) return no( AA_ERR_ARGUMENT, i, "null pointer" );
  aa_stream * s = j.stream;
  if ( s->ctx != ctx ) return no( AA_ERR_ARGUMENT, i, "stream belongs to another context" );
  for ( int k = 0; k < i; k++ ) if ( jobs[k].stream == s ) return no( AA_ERR_ARGUMENT, i, "its stream is also job " + std::to_string( k ) + "'s: one new frame per stream and call" );
  const bool key = j.hdr->key_frame != 0;
  if ( key && !Call::kForward ) return no( AA_ERR_ARGUMENT, i, "the new frame's header says key frame: a re-encode makes an inter frame" );
  if ( j.hdr->segmentation_enabled ) return no( AA_ERR_UNSUPPORTED, i, "segmentation is enabled: the reference refuses it too (reencode.cc:47-49)" );
  if ( j.quality != AA_REENCODE_BEST && j.quality != AA_REENCODE_REALTIME ) return no( AA_ERR_ARGUMENT, i, "quality is neither AA_REENCODE_BEST nor AA_REENCODE_REALTIME" );
  const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
  if ( j.hdr->mb_width != s->parser.mb_width() || j.hdr->mb_height != s->parser.mb_height() || j.hdr->num_macroblocks != nmb )
    return no( AA_ERR_ARGUMENT, i, "the header's macroblock dimensions are not this decoder's" );
  // (a key frame predicts from nothing: it needs neither a reference nor a stream whose frames are all decoded)
  if ( !key && s->next_submit != static_cast<int>( s->frames.size() ) ) return no( AA_ERR_LOGIC, i, "its stream holds a frame that is appended but not decoded: the references are not current" );
  if ( j.target.y_stride < int64_t( s->pw ) || j.target.uv_stride < int64_t( s->pw / 2 ) ) return no( AA_ERR_ARGUMENT, i, "row stride smaller than the padded plane's width" );
  for ( int f = 0; f < 6; f++ ) if ( !j.hdr->quant[0][f] ) return no( AA_ERR_ARGUMENT, i, "a quantiser factor of the header is zero" );
  if ( !key && ( s->cur_ref_slot[0] < 0 || !s->slots[s->cur_ref_slot[0]].dev ) ) return no( AA_ERR_LOGIC, i, "its stream has no reference rasters" );
  if ( Call::kForward && !key && s->slots[s->cur_ref_slot[0]].shared )
    return no( AA_ERR_LOGIC, i, "its stream has no decoded last reference (the blank raster of a new decoder): an inter frame needs a key frame before it" );
  return AA_OK;
}

// aa_encode_two_pass_batch / aa_encode_two_pass_device_batch: which jobs of the call are two-pass key jobs (flags, one byte per job) and
// where each job's first-pass token_prob_update goes (updates, AA_TWO_PASS_UPDATES bytes per job).  Every other call: none.
struct TwoPassArgs {
  const uint8_t * flags = nullptr;
  uint8_t * updates = nullptr;
  template <class Job> bool two( const Job & j, int i ) const { return flags && flags[i] && j.hdr->key_frame; }
};
// A two-pass key job's cost block: EncKey2Costs (whose head is the first pass's EncKeyCosts: one table entry serves k_encode_key and
// k_encode_key2) | the token costs | the first pass's branch counts | its updates | the macroblocks' side bits
struct Key2Block {
  size_t trellis, counts, updates, bits, bytes;
  explicit Key2Block( size_t nmb )
  {
    trellis = align_up( sizeof( aa::EncKey2Costs ) ); counts = trellis + align_up( sizeof( aa::TrellisCosts ) ); updates = counts + align_up( 2112 * sizeof( uint32_t ) );
    bits = updates + align_up( AA_TWO_PASS_UPDATES ); bytes = bits + align_up( nmb );
  }
};
const aa::TrellisCosts & trellis_costs()
{
  static const aa::TrellisCosts T = [] { aa::TrellisCosts t; aa::trellis_fill_costs( t ); return t; }();
  return T;
}
void fill_key2_block( uint8_t * host, uint8_t * dev, size_t nmb, uint16_t y_ac )
{
  const Key2Block at( nmb );
  std::memset( host, 0, at.bytes );
  aa::EncKey2Costs & C = *reinterpret_cast<aa::EncKey2Costs *>( host );
  aa::enc_fill_key_costs( C.enc, y_ac );
  std::memcpy( host + at.trellis, &trellis_costs(), sizeof( aa::TrellisCosts ) );
  C.trellis = reinterpret_cast<const aa::TrellisCosts *>( dev + at.trellis );
  C.counts = reinterpret_cast<uint32_t *>( dev + at.counts );
  C.updates = dev + at.updates;
  C.first_pass = dev + at.bits;
  C.census = nullptr;
}

// Where a slice's kernels find and leave one job's data, in the slice's piece
struct ReencodePlaces { uint8_t * costs, * masks, * records, * dense, * side, * raster; };

// What a slice's kernels read of one job, into its entry of the job table, its rate model (the pinned copy of *at.costs) and what
// mb_lf_level reads of it: the new header's level, the stream's current adjustments where the header keeps them switched on
template <class Call, class Job>
void reencode_fill_job( aa_reencode_dev_job & d, void * costs, aa::HeaderParams & fp, const Job & j, const ReencodePlaces & at, bool two = false )
{
  aa_stream * s = j.stream;
  const bool key = Call::kForward && j.hdr->key_frame;
  std::memset( &d, 0, sizeof d );
  if ( !key ) for ( int p = 0; p < 3; p++ ) d.base.ref[1][p] = slot_plane( s, s->cur_ref_slot[0], p );          // every candidate predicts from LAST
  d.base.target[0] = static_cast<const uint8_t *>( j.target.y ); d.base.target[1] = static_cast<const uint8_t *>( j.target.u ); d.base.target[2] = static_cast<const uint8_t *>( j.target.v );
  d.base.target_stride[0] = j.target.y_stride; d.base.target_stride[1] = j.target.uv_stride;
  // the rate model: the mode costs are constants, the vector costs come from the stream's CURRENT probabilities (reencode.cc:82-84)
  // (the forward encoder adds the job's multipliers and the search's site costs; a key frame's block holds no vector cost at all)
  if ( !Call::kForward ) aa::reenc_fill_costs( *static_cast<aa::ReencCosts *>( costs ), s->parser.probs().mv, j.quality );
  else if ( key && two ) fill_key2_block( static_cast<uint8_t *>( costs ), at.costs, size_t( j.hdr->mb_width ) * j.hdr->mb_height, j.hdr->quant[0][1] );
  else if ( key ) aa::enc_fill_key_costs( *static_cast<aa::EncKeyCosts *>( costs ), j.hdr->quant[0][1] );
  else aa::enc_fill_inter_costs( *static_cast<aa::EncInterCosts *>( costs ), s->parser.probs().mv, j.quality, j.hdr->quant[0][1], j.hdr->q_index );
  d.costs = at.costs;
  d.base.masks = reinterpret_cast<uint32_t *>( at.masks );
  d.mbs_out = reinterpret_cast<aa_mb_info *>( at.records );
  d.base.coeffs = reinterpret_cast<int16_t *>( at.dense );
  d.nb = reinterpret_cast<uint32_t *>( at.side );
  d.base.recon[0] = at.raster; d.base.recon[1] = at.raster + s->plane_bytes[0]; d.base.recon[2] = at.raster + s->plane_bytes[0] + s->plane_bytes[1];
  std::memcpy( d.base.quant, j.hdr->quant[0], sizeof d.base.quant );
  d.base.mbw = j.hdr->mb_width; d.base.mbh = j.hdr->mb_height; d.base.has_intra = 1;
  const aa::FilterAdjustState & fa = s->parser.filter_adjustments();
  // (a key frame resets the stream's adjustments, and aa_frame_header carries no deltas of its own: its level stands unadjusted)
  aa::compact::lf_params( fp, j.hdr->loop_filter_level, !key && j.hdr->filter_adjustments_enabled && fa.enabled, fa.ref, fa.mode );
}

// A job's cost block in the slice's upload, and a slice's table order: two-pass key jobs first, then the other key jobs, so that each
// kernel finds its kind in one run
template <class Call, class Job>
size_t reencode_costs_bytes( const Job & j, bool two = false )
{
  if ( !Call::kForward ) return align_up( sizeof( aa::ReencCosts ) );
  if ( two ) return Key2Block( size_t( j.hdr->mb_width ) * j.hdr->mb_height ).bytes;
  return align_up( j.hdr->key_frame ? sizeof( aa::EncKeyCosts ) : sizeof( aa::EncInterCosts ) );
}
template <class Call, class Job>
int reencode_slice_order( const Job * jobs, int first, int count, std::vector<int> & at, const TwoPassArgs & tp = TwoPassArgs(), int * keys2 = nullptr )
{
  at.clear();
  if ( Call::kForward ) for ( int k = 0; k < count; k++ ) if ( tp.two( jobs[first + k], first + k ) ) at.push_back( first + k );
  if ( keys2 ) *keys2 = static_cast<int>( at.size() );
  if ( Call::kForward ) for ( int k = 0; k < count; k++ ) if ( jobs[first + k].hdr->key_frame && !tp.two( jobs[first + k], first + k ) ) at.push_back( first + k );
  const int keys = static_cast<int>( at.size() );
  for ( int k = 0; k < count; k++ ) if ( !( Call::kForward && jobs[first + k].hdr->key_frame ) ) at.push_back( first + k );
  return keys;
}
// The decision over a slice's table: k_reencode_inter, or k_encode_key over its first `keys` entries -- behind it, over the first `keys2`
// of them, what lies between the passes and k_encode_key2 -- and k_encode_inter over the rest
template <class Call>
aa_status reencode_launch_decision( aa_ctx * ctx, const aa_reencode_dev_job * table, int count, int keys, int keys2 = 0, uint32_t max_mbs2 = 0 )
{
  if ( !Call::kForward ) {
    if ( int e = aa::launch_reencode( table, count, ctx->reenc_slots, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_reencode_inter" );
    return AA_OK;
  }
  if ( keys ) if ( int e = aa::launch_encode( table, keys, true, ctx->reenc_slots, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_encode_key" );
  if ( keys2 ) if ( int e = aa::launch_encode_second_pass( table, keys2, max_mbs2, ctx->reenc_slots, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_key2_first_pass / k_key2_updates / k_encode_key2" );
  if ( count > keys ) if ( int e = aa::launch_encode( table + keys, count - keys, false, ctx->reenc_slots, ctx->compute ) ) return hip_fail( static_cast<hipError_t>( e ), "k_encode_inter" );
  return AA_OK;
}
// The first pass's updates of a slice's two-pass jobs (its first keys2 table entries) into the caller's array, queued behind the kernels;
// every other job's entry is zero: no update
template <class Job>
aa_status reencode_fetch_updates( aa_ctx * ctx, const TwoPassArgs & tp, const Job * jobs, const std::vector<int> & at_job, int keys2, const std::vector<uint8_t *> & dev_costs )
{
  if ( !tp.updates ) return AA_OK;
  for ( size_t k = 0; k < at_job.size(); k++ ) {
    uint8_t * out = tp.updates + size_t( at_job[k] ) * AA_TWO_PASS_UPDATES;
    if ( static_cast<int>( k ) >= keys2 ) { std::memset( out, 0, AA_TWO_PASS_UPDATES ); continue; }
    const Job & j = jobs[at_job[k]];
    HIP_TRY( hipMemcpyAsync( out, dev_costs[k] + Key2Block( size_t( j.hdr->mb_width ) * j.hdr->mb_height ).updates, AA_TWO_PASS_UPDATES, hipMemcpyDeviceToHost, ctx->compute ) );
  }
  return AA_OK;
}

} // namespace

extern "C" {

aa_status aa_ctx_set_reencode_slots( aa_ctx * ctx, int slots )
{
  if ( !ctx || slots < 1 || slots > 16 ) return fail( AA_ERR_ARGUMENT, "aa_ctx_set_reencode_slots: 1..16 macroblocks of an anti-diagonal per round" );
  ctx->reenc_slots = slots;
  return AA_OK;
}

} // extern "C"

namespace {

template <class Call>
aa_status reencode_batch( aa_ctx * ctx, aa_reencode_job * jobs, int n, const TwoPassArgs tp = TwoPassArgs() )
{
  const std::string who = Call::kHost;
  const auto no = [&who]( aa_status code, int i, const std::string & what ) { return fail( code, who + ": job " + std::to_string( i ) + ": " + what ); };
  if ( !ctx || !jobs || n <= 0 ) return fail( AA_ERR_ARGUMENT, who + ": bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  // ---- 1. the arguments: nothing is launched, nothing appended unless every job of the call is good ----
  for ( int i = 0; i < n; i++ ) {
    aa_reencode_job & j = jobs[i];
    if ( !j.mbs_out || ( !j.coeffs_out && j.coeff_capacity_blocks ) ) return no( AA_ERR_ARGUMENT, i, "null pointer" );
    if ( aa_status st = reencode_check_job<Call>( Call::kHost, ctx, jobs, i ) ) return st;
    j.num_coeff_blocks = 0; j.frame_index = -1;
  }

  const double t_call = now_ms();
  double ms_kernels = 0, ms_download = 0, ms_records = 0;
  // ---- 2..5. slice by slice: job table and rate models up, the kernel, records, coefficients and masks down, records into the caller's arrays ----
  const size_t share = rebase_slice_bytes( ctx );
  std::vector<uint32_t> intra_mbs( n, 0 );
  for ( int first = 0; first < n; ) {
    int count = 0;
    size_t dense_total = 0, masks_total = 0, records_total = 0, side_total = 0, raster_total = 0, costs_total = 0;
    while ( first + count < n ) {
      const aa_stream * s = jobs[first + count].stream;
      const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
      if ( count && dense_total + nmb * AA_REBASE_MB_BYTES > share ) break;
      dense_total += align_up( nmb * AA_REBASE_MB_BYTES ); masks_total += align_up( nmb * sizeof( uint32_t ) );
      records_total += align_up( nmb * sizeof( aa_mb_info ) ); side_total += align_up( nmb * sizeof( aa::ReencNeighbour ) );
      raster_total += s->slot_bytes; costs_total += reencode_costs_bytes<Call>( jobs[first + count], tp.two( jobs[first + count], first + count ) );
      count++;
    }
    std::vector<int> at_job;                     // table entry -> job of the call
    int keys2 = 0;
    const int keys = reencode_slice_order<Call>( jobs, first, count, at_job, tp, &keys2 );
    std::vector<uint8_t *> dev_costs( count );   // a table entry's cost block on the device
    uint32_t max_mbs2 = 0;                       // the largest frame among the two-pass jobs
    // the pinned side: job table | every job's rate model (a JobRing entry, read by one copy); the device piece: the same, then per job
    // masks | records | dense coefficients (the results, downloaded by one copy), then side records and reconstruction rasters
    const size_t table_bytes = align_up( size_t( count ) * sizeof( aa_reencode_dev_job ) );
    const size_t up_bytes = table_bytes + costs_total, result_bytes = masks_total + records_total + dense_total;
    const size_t piece_bytes = up_bytes + result_bytes + side_total + raster_total;
    JobRing::Entry * rb = nullptr;
    if ( aa_status st = ctx->rebase_ring.take( up_bytes, align_up( 64 * sizeof( aa_rebase_dev_job ) ), &rb ) ) return st;
    uint8_t * piece = nullptr;
    if ( aa_status st = dev_alloc_compute( ctx, piece_bytes, &piece ) ) return st;
    struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { dev_free_compute( c, p, b ); } } back { ctx, piece, piece_bytes };
    size_t staging_bytes = 0;
    uint8_t * staging = pinned_get( ctx, result_bytes, &staging_bytes );
    if ( !staging ) return fail( AA_ERR_HIP, who + ": pinned staging allocation failed" );
    struct Unpin { aa_ctx * c; uint8_t * p; size_t b; ~Unpin() { std::lock_guard<std::mutex> g( c->pool_mu ); c->pinned_pool.emplace_back( p, b ); } } unpin { ctx, staging, staging_bytes };

    aa_reencode_dev_job * table = reinterpret_cast<aa_reencode_dev_job *>( rb->host );
    std::vector<size_t> result_off( count );
    std::vector<aa::HeaderParams> lf_params( count );
    size_t up_off = table_bytes, res_off = 0, side_off = up_bytes + result_bytes;
    for ( int k = 0; k < count; k++ ) {
      const aa_reencode_job & j = jobs[at_job[k]];
      aa_stream * s = j.stream;
      const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
      ReencodePlaces at;
      at.costs = piece + up_off;
      result_off[k] = res_off;
      at.masks = piece + up_bytes + res_off; res_off += align_up( nmb * sizeof( uint32_t ) );
      at.records = piece + up_bytes + res_off; res_off += align_up( nmb * sizeof( aa_mb_info ) );
      at.dense = piece + up_bytes + res_off; res_off += align_up( nmb * AA_REBASE_MB_BYTES );
      at.side = piece + side_off; side_off += align_up( nmb * sizeof( aa::ReencNeighbour ) );
      at.raster = piece + side_off; side_off += s->slot_bytes;
      dev_costs[k] = at.costs;
      if ( k < keys2 ) max_mbs2 = std::max<uint32_t>( max_mbs2, static_cast<uint32_t>( nmb ) );
      reencode_fill_job<Call>( table[k], rb->host + up_off, lf_params[k], j, at, k < keys2 );
      up_off += reencode_costs_bytes<Call>( j, k < keys2 );
    }
    hipEvent_t ev[3] = { get_event( ctx ), get_event( ctx ), get_event( ctx ) };      // (aa_reencode_last_timing: tables up + kernel, results down)
    struct Events { aa_ctx * c; hipEvent_t * e; ~Events() { for ( int i = 0; i < 3; i++ ) if ( e[i] ) c->free_events.push_back( e[i] ); } } events { ctx, ev };
    if ( !ev[0] || !ev[1] || !ev[2] ) return fail( AA_ERR_HIP, who + ": hipEventCreate failed" );
    HIP_TRY( hipEventRecord( ev[0], ctx->compute ) );
    HIP_TRY( hipMemcpyAsync( piece, rb->host, up_bytes, hipMemcpyHostToDevice, ctx->compute ) );
    if ( aa_status st = ctx->rebase_ring.mark( *rb, ctx->compute ) ) return st;
    if ( aa_status st = reencode_launch_decision<Call>( ctx, reinterpret_cast<const aa_reencode_dev_job *>( piece ), count, keys, keys2, max_mbs2 ) ) return st;
    HIP_TRY( hipEventRecord( ev[1], ctx->compute ) );
    if ( aa_status st = reencode_fetch_updates( ctx, tp, jobs, at_job, keys2, dev_costs ) ) return st;
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
        aa_reencode_job & j = jobs[at_job[k]];
        const size_t nmb = size_t( j.hdr->mb_width ) * j.hdr->mb_height;
        const uint8_t * at = staging + result_off[k];
        const uint32_t * masks = reinterpret_cast<const uint32_t *>( at ); at += align_up( nmb * sizeof( uint32_t ) );
        const aa_mb_info * recs = reinterpret_cast<const aa_mb_info *>( at ); at += align_up( nmb * sizeof( aa_mb_info ) );
        const int16_t * dense = reinterpret_cast<const int16_t *>( at );
        const RebaseCounts need = reencode_records( recs, masks, dense, nmb, lf_params[k], nullptr, nullptr );
        j.num_coeff_blocks = need.blocks; intra_mbs[at_job[k]] = need.intra;
        if ( need.blocks > j.coeff_capacity_blocks ) { int none = -1; short_job.compare_exchange_strong( none, at_job[k] ); continue; }
        reencode_records( recs, masks, dense, nmb, lf_params[k], j.mbs_out, j.coeffs_out );
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

  // ---- 6. the frames whose job says so join their streams, as aa_stream_append_records appends them ----
  const double t_append = now_ms();
  {
    std::vector<aa_status> status( n, AA_OK );
    std::vector<std::string> message( n );
    std::atomic<int> next { 0 };
    auto work = [&]() {
      (void) hipSetDevice( ctx->device );
      for ( ;; ) {
        const int i = next.fetch_add( 1 );
        if ( i >= n ) return;
        aa_reencode_job & j = jobs[i];
        if ( !j.append ) continue;
        aa_frame_header h = *j.hdr;
        h.key_frame = Call::kForward && j.hdr->key_frame ? 1 : 0; h.num_coeff_blocks = j.num_coeff_blocks;
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
  std::memcpy( Call::timing( ctx ), timing, sizeof timing );
  return AA_OK;
}

/* The re-encode with the new frame's records kept in HBM: the kernel of aa_reencode_batch, then k_reencode_count / k_reencode_compact
 * (reencode_compact_kernels.hip) in place of the download, reencode_records and the append -- aa_rebase_device_batch's scheme.  The
 * decision's modes are known on the device only, so the count pass also makes every frame's intra-row words; per slice one small copy
 * brings the blocks stored per run of 256 macroblocks and those words down, and the host derives from them what it reads off the
 * input records of a rebase: the block count and the piece's size, the intra count, the intra diagonals.  The appended FrameRec is a
 * device-rebased frame's: no chunk, no batch, rec_block = the piece (job record | macroblock records | intra-row words | dense
 * blocks), dev_job = its start. */
template <class Call>
aa_status reencode_device_batch( aa_ctx * ctx, aa_reencode_device_job * jobs, int n, const TwoPassArgs tp = TwoPassArgs() )
{
  const std::string who = Call::kDevice;
  if ( !ctx || !jobs || n <= 0 ) return fail( AA_ERR_ARGUMENT, who + ": bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  // ---- 1. the arguments: nothing is launched, nothing appended unless every job of the call is good ----
  for ( int i = 0; i < n; i++ ) {
    if ( aa_status st = reencode_check_job<Call>( Call::kDevice, ctx, jobs, i ) ) return st;
    jobs[i].num_coeff_blocks = 0; jobs[i].num_intra_mbs = 0; jobs[i].frame_index = -1;
  }

  const double t_call = now_ms();
  // the frames in the making and their pieces, which go back to the pool unless the whole call succeeds (through an epoch:
  // k_reencode_compact may be queued on them)
  struct Made { FrameRec rec; uint8_t * piece = nullptr; size_t bytes = 0; };
  std::vector<Made> made( n );
  struct GiveBack { aa_ctx * c; std::vector<Made> & m; bool keep = false;
                    ~GiveBack() { if ( !keep ) for ( Made & x : m ) dev_free( c, x.piece, x.bytes, true ); } } give_back { ctx, made };
  std::vector<hipEvent_t> events;            // five per slice: [0..1] tables up, the decision, the count; [1..2] sums and row words down; [3..4] second table up, compaction
  struct Events { aa_ctx * c; std::vector<hipEvent_t> & e; ~Events() { for ( hipEvent_t x : e ) if ( x ) c->free_events.push_back( x ); } } events_back { ctx, events };

  // ---- 2..5. slice by slice: job table and rate models up, the decision and the count, sums and row words down, pieces, the compaction ----
  const size_t share = rebase_slice_bytes( ctx );
  const size_t job_bytes = align_up( sizeof( aa_dev_frame ) );
  for ( int first = 0; first < n; ) {
    int count = 0;
    size_t dense_total = 0, masks_total = 0, records_total = 0, side_total = 0, raster_total = 0, rows_total = 0, costs_total = 0;
    uint32_t max_mbs = 0;
    while ( first + count < n ) {
      const aa_stream * s = jobs[first + count].stream;
      const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
      if ( count && dense_total + nmb * AA_REBASE_MB_BYTES > share ) break;
      dense_total += align_up( nmb * AA_REBASE_MB_BYTES ); masks_total += align_up( nmb * sizeof( uint32_t ) );
      records_total += align_up( nmb * sizeof( aa_mb_info ) ); side_total += align_up( nmb * sizeof( aa::ReencNeighbour ) );
      rows_total += align_up( size_t( aa::compact::row_words( s->parser.mb_width(), s->parser.mb_height() ) ) * sizeof( unsigned long long ) );
      raster_total += s->slot_bytes; costs_total += reencode_costs_bytes<Call>( jobs[first + count], tp.two( jobs[first + count], first + count ) );
      max_mbs = std::max<uint32_t>( max_mbs, static_cast<uint32_t>( nmb ) );
      count++;
    }
    std::vector<int> at_job;                     // table entry -> job of the call
    int keys2 = 0;
    const int keys = reencode_slice_order<Call>( jobs, first, count, at_job, tp, &keys2 );
    std::vector<uint8_t *> dev_costs( count );   // a table entry's cost block on the device
    uint32_t max_mbs2 = 0;                       // the largest frame among the two-pass jobs
    // the slice's piece: job table | rate models (one upload) | compaction table | filter-level parameters (a second one, once the
    // pieces are known) | partial sums | intra-row words (one download) | masks | records | dense slots | side records | reconstruction
    // rasters.  Pinned: a JobRing entry for each upload; the download lands behind the first one's table.
    const uint32_t stride = aa::compact::runs_of( max_mbs );
    const size_t table_bytes = align_up( size_t( count ) * sizeof( aa_reencode_dev_job ) );
    const size_t up_bytes = table_bytes + costs_total;
    const size_t ctable_bytes = align_up( size_t( count ) * sizeof( aa_rebase_compact_job ) );
    const size_t up2_bytes = ctable_bytes + align_up( size_t( count ) * sizeof( aa::HeaderParams ) );
    const size_t partial_bytes = align_up( size_t( count ) * stride * sizeof( uint32_t ) );
    const size_t down_bytes = partial_bytes + rows_total;
    const size_t result_bytes = masks_total + records_total + dense_total;
    const size_t piece_bytes = up_bytes + up2_bytes + down_bytes + result_bytes + side_total + raster_total;
    JobRing::Entry * rb = nullptr, * rb2 = nullptr;
    if ( aa_status st = ctx->rebase_ring.take( up_bytes + down_bytes, align_up( 64 * sizeof( aa_rebase_dev_job ) ), &rb ) ) return st;
    if ( aa_status st = ctx->rebase_ring.take( up2_bytes, align_up( 64 * sizeof( aa_rebase_compact_job ) ), &rb2 ) ) return st;
    uint8_t * piece = nullptr;
    if ( aa_status st = dev_alloc_compute( ctx, piece_bytes, &piece ) ) return st;
    struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { dev_free_compute( c, p, b ); } } back { ctx, piece, piece_bytes };
    uint8_t * const piece2 = piece + up_bytes;
    uint8_t * const down_dev = piece2 + up2_bytes;
    uint32_t * const partials_dev = reinterpret_cast<uint32_t *>( down_dev );
    uint8_t * const results = down_dev + down_bytes;

    aa_reencode_dev_job * table = reinterpret_cast<aa_reencode_dev_job *>( rb->host );
    aa_rebase_compact_job * ctable = reinterpret_cast<aa_rebase_compact_job *>( rb2->host );
    aa::HeaderParams * lf_params = reinterpret_cast<aa::HeaderParams *>( rb2->host + ctable_bytes );
    std::vector<size_t> rows_at( count );      // a job's intra-row words, from the download's start
    size_t up_off = table_bytes, rows_off = partial_bytes, res_off = 0, side_off = up_bytes + up2_bytes + down_bytes + result_bytes;
    for ( int k = 0; k < count; k++ ) {
      const aa_reencode_device_job & j = jobs[at_job[k]];
      aa_stream * s = j.stream;
      const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
      ReencodePlaces at;
      at.costs = piece + up_off;
      at.masks = results + res_off; res_off += align_up( nmb * sizeof( uint32_t ) );
      at.records = results + res_off; res_off += align_up( nmb * sizeof( aa_mb_info ) );
      at.dense = results + res_off; res_off += align_up( nmb * AA_REBASE_MB_BYTES );
      at.side = piece + side_off; side_off += align_up( nmb * sizeof( aa::ReencNeighbour ) );
      at.raster = piece + side_off; side_off += s->slot_bytes;
      dev_costs[k] = at.costs;
      if ( k < keys2 ) max_mbs2 = std::max<uint32_t>( max_mbs2, static_cast<uint32_t>( nmb ) );
      reencode_fill_job<Call>( table[k], rb->host + up_off, lf_params[k], j, at, k < keys2 );
      up_off += reencode_costs_bytes<Call>( j, k < keys2 );
      const uint32_t words = aa::compact::row_words( j.hdr->mb_width, j.hdr->mb_height );
      table[k].intra_rows = reinterpret_cast<unsigned long long *>( down_dev + rows_off );
      rows_at[k] = rows_off;
      rows_off += align_up( size_t( words ) * sizeof( unsigned long long ) );
      aa_rebase_compact_job & o = ctable[k];
      std::memset( &o, 0, sizeof o );
      o.rows = table[k].intra_rows;
      o.rows_words = words;
    }
    hipEvent_t ev[5] = { get_event( ctx ), get_event( ctx ), get_event( ctx ), get_event( ctx ), get_event( ctx ) };
    events.insert( events.end(), ev, ev + 5 );
    if ( !ev[0] || !ev[1] || !ev[2] || !ev[3] || !ev[4] ) return fail( AA_ERR_HIP, who + ": hipEventCreate failed" );
    HIP_TRY( hipEventRecord( ev[0], ctx->compute ) );
    HIP_TRY( hipMemcpyAsync( piece, rb->host, up_bytes, hipMemcpyHostToDevice, ctx->compute ) );
    if ( aa_status st = reencode_launch_decision<Call>( ctx, reinterpret_cast<const aa_reencode_dev_job *>( piece ), count, keys, keys2, max_mbs2 ) ) return st;
    if ( aa_status st = reencode_fetch_updates( ctx, tp, jobs, at_job, keys2, dev_costs ) ) return st;
    if ( int e = aa::launch_reencode_count( reinterpret_cast<const aa_reencode_dev_job *>( piece ), count, max_mbs, partials_dev, stride, ctx->compute ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_reencode_count" );
    HIP_TRY( hipEventRecord( ev[1], ctx->compute ) );
    const uint8_t * const down = rb->host + up_bytes;
    const uint32_t * const partials = reinterpret_cast<const uint32_t *>( down );
    HIP_TRY( hipMemcpyAsync( rb->host + up_bytes, down_dev, down_bytes, hipMemcpyDeviceToHost, ctx->compute ) );
    HIP_TRY( hipEventRecord( ev[2], ctx->compute ) );
    if ( aa_status st = ctx->rebase_ring.mark( *rb, ctx->compute ) ) return st;
    HIP_TRY( hipStreamSynchronize( ctx->compute ) );
    if ( aa_status st = check_watchdog( ctx ) ) return st;

    // every frame's block count and intra macroblocks, its piece at that size, and where the second kernel puts what
    for ( int k = 0; k < count; k++ ) {
      aa_reencode_device_job & j = jobs[at_job[k]];
      Made & m = made[at_job[k]];
      const uint32_t mbw = j.hdr->mb_width, mbh = j.hdr->mb_height;
      const size_t nmb = size_t( mbw ) * mbh;
      aa_rebase_compact_job & o = ctable[k];
      uint32_t blocks = 0;
      for ( uint32_t r = 0; r < aa::compact::runs_of( static_cast<uint32_t>( nmb ) ); r++ ) blocks += partials[size_t( k ) * stride + r];
      if ( blocks > nmb * 25 ) return fail( AA_ERR_HIP, who + ": job " + std::to_string( at_job[k] ) + ": k_reencode_count reports more blocks than the frame can hold" );
      const unsigned long long * rows = reinterpret_cast<const unsigned long long *>( down + rows_at[k] );
      FrameRec & rec = m.rec;
      rec.intra_diagonals.assign( mbw + 2 * ( mbh - 1 ), 0 );
      aa::compact::intra_diagonals( rows, mbw, mbh, rec.intra_diagonals.data() );
      rec.has_split = false;                   // (the decision never chooses SPLITMV)
      j.num_coeff_blocks = blocks; j.num_intra_mbs = aa::compact::intra_count( rows, o.rows_words );
      const size_t mb_bytes = align_up( nmb * sizeof( aa_mb_info ) );
      const size_t rows_bytes = align_up( size_t( o.rows_words ) * sizeof( unsigned long long ) );
      m.bytes = rebase_piece_bytes( job_bytes + mb_bytes + rows_bytes + align_up( size_t( blocks ) * 32 ) );
      if ( aa_status st = dev_alloc( ctx, m.bytes, &m.piece ) ) return st;
      rec.hdr = *j.hdr;
      rec.hdr.key_frame = Call::kForward && j.hdr->key_frame ? 1 : 0; rec.hdr.num_coeff_blocks = blocks;
      rec.hdr.num_intra_mbs = j.num_intra_mbs; rec.hdr.has_intra_mb = j.num_intra_mbs != 0;
      rec.rec_block = m.piece; rec.rec_bytes = m.bytes;
      rec.dev_job = reinterpret_cast<const aa_dev_frame *>( m.piece );
      rec.dev_mbs = reinterpret_cast<aa_mb_info *>( m.piece + job_bytes );
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
    if ( int e = aa::launch_reencode_compact( reinterpret_cast<const aa_reencode_dev_job *>( piece ), reinterpret_cast<const aa_rebase_compact_job *>( piece2 ), piece2 + ctable_bytes, count,
                                              max_mbs, partials_dev, stride, ctx->compute ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_reencode_compact" );
    HIP_TRY( hipEventRecord( ev[4], ctx->compute ) );
    if ( aa_status st = ctx->rebase_ring.mark( *rb2, ctx->compute ) ) return st;
    first += count;
  }
  // the call is synchronous, as aa_reencode_batch is: whoever reads the pieces next finds them written
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
  std::memcpy( Call::timing( ctx ), timing, sizeof timing );
  return AA_OK;
}

} // namespace

extern "C" {

aa_status aa_reencode_batch( aa_ctx * ctx, aa_reencode_job * jobs, int n ) { return reencode_batch<ReencodeCall>( ctx, jobs, n ); }
aa_status aa_reencode_device_batch( aa_ctx * ctx, aa_reencode_device_job * jobs, int n ) { return reencode_device_batch<ReencodeCall>( ctx, jobs, n ); }

aa_status aa_reencode_last_timing( aa_ctx * ctx, double out[5] )
{
  if ( !ctx || !out ) return fail( AA_ERR_ARGUMENT, "aa_reencode_last_timing: null argument" );
  std::memcpy( out, ctx->reencode_timing, sizeof ctx->reencode_timing );
  return AA_OK;
}

} // extern "C"
