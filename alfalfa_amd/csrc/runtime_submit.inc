// runtime.cpp, one of its pieces (ABI): frames coming in -- host-parsed frames and frames given as records, aa_submit_frames (routing: GPU lanes,
// host lanes, a worker per stream), the hand-over to the token workers, the host lanes' worker threads.
namespace {
// A frame whose records are produced on the HOST -- by the bitstream parser (aa_stream_parse) or handed in as records
// (aa_stream_append_records) -- is staged in the stream's pinned chunk (mirrored 1:1 in HBM, uploaded by aa_stream_upload):
// job record | macroblock records | intra row masks | coefficient blocks.  `fill` writes the header, the macroblock records and
// the coefficient blocks into the staging area it is given (worst-case sized) or throws aa::ParseError.
template <class Fill>
aa_status append_host_frame( aa_stream * s, int * frame_index, aa_frame_header * hdr_out, Fill && fill )
{
  if ( aa_status st = set_device( s->ctx ) ) return st;
  const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
  const size_t job_bytes = align_up( sizeof( aa_dev_frame ) );
  const size_t mb_bytes = align_up( nmb * sizeof( aa_mb_info ) );
  const size_t words_per_row = ( s->parser.mb_width() + 63 ) / 64;
  const size_t rows_bytes = align_up( words_per_row * s->parser.mb_height() * sizeof( unsigned long long ) );
  const size_t worst = job_bytes + mb_bytes + rows_bytes + align_up( nmb * 25 * 32 );
  Chunk * c;
  if ( aa_status st = reserve( s, worst, &c ) ) return st;
  const size_t off = c->used;
  aa_dev_frame * job = reinterpret_cast<aa_dev_frame *>( c->host + off );
  aa_mb_info * mbs = reinterpret_cast<aa_mb_info *>( c->host + off + job_bytes );
  unsigned long long * intra_rows = reinterpret_cast<unsigned long long *>( c->host + off + job_bytes + mb_bytes );
  int16_t * coeffs = reinterpret_cast<int16_t *>( c->host + off + job_bytes + mb_bytes + rows_bytes );

  FrameRec rec;
  try { fill( rec.hdr, mbs, coeffs ); }
  catch ( const aa::ParseError & e ) { return fail( e.code, e.message ); }
  const aa_frame_header & h = rec.hdr;
  c->used = off + job_bytes + mb_bytes + rows_bytes + align_up( size_t( h.num_coeff_blocks ) * 32 );   // commit what was used

  // which 2:1 anti-diagonals hold intra MBs (launch schedule of k_recon_intra)
  const int mbw = h.mb_width, mbh = h.mb_height;
  rec.intra_diagonals.assign( mbw + 2 * ( mbh - 1 ), 0 );
  std::memset( intra_rows, 0, words_per_row * mbh * sizeof( unsigned long long ) );
  if ( h.has_intra_mb )
    for ( int r = 0; r < mbh; r++ ) for ( int col = 0; col < mbw; col++ )
      if ( !( mbs[r * mbw + col].flags & AA_MB_INTER ) ) {
        rec.intra_diagonals[col + 2 * r] = 1;
        intra_rows[r * words_per_row + ( col >> 6 )] |= 1ull << ( col & 63 );
      }

  if ( !h.key_frame )
    for ( size_t i = 0; i < nmb; i++ ) if ( mbs[i].y_mode == 9 /* SPLITMV */ ) { rec.has_split = true; break; }

  fill_job( rec, job );
  job->mbs = reinterpret_cast<const aa_mb_info *>( c->dev + off + job_bytes );
  job->intra_rows = reinterpret_cast<const unsigned long long *>( c->dev + off + job_bytes + mb_bytes );
  job->coeffs = reinterpret_cast<const int16_t *>( c->dev + off + job_bytes + mb_bytes + rows_bytes );
  rec.host_job = job;
  rec.dev_job = reinterpret_cast<const aa_dev_frame *>( c->dev + off );
  rec.chunk = static_cast<int>( c - s->chunks.data() );
  c->live_frames++;
  const int fi = static_cast<int>( s->frames.size() );
  s->frames.push_back( std::move( rec ) );
  if ( frame_index ) *frame_index = fi;
  if ( hdr_out ) *hdr_out = h;
  return AA_OK;
}
} // namespace
extern "C" {

aa_status aa_stream_parse( aa_stream * s, const uint8_t * data, size_t size, int * frame_index, aa_frame_header * hdr_out )
{
  if ( !s || !data ) return fail( AA_ERR_ARGUMENT, "aa_stream_parse: null argument" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  if ( aa_status st = segmap_to_host( s ) ) return st;
  return append_host_frame( s, frame_index, hdr_out, [&]( aa_frame_header & hdr, aa_mb_info * mbs, int16_t * coeffs ) { s->parser.parse( data, size, hdr, mbs, coeffs ); } );
}

/* A frame given as RECORDS, no bitstream: what Encoder::write_frame has in hand when it updates its references
 * (encoder.cc:146-160: frame.decode + frame.loopfilter + copy_to on a Frame it holds), and what xc-enc -r replays. */
aa_status aa_stream_append_records( aa_stream * s, const aa_frame_header * hdr, const aa_mb_info * mbs_in, const int16_t * coeffs_in, int * frame_index )
{
  if ( !s || !hdr || !mbs_in ) return fail( AA_ERR_ARGUMENT, "aa_stream_append_records: null argument" );
  if ( hdr->num_coeff_blocks && !coeffs_in ) return fail( AA_ERR_ARGUMENT, "aa_stream_append_records: coefficient blocks missing" );
  const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
  if ( hdr->mb_width != s->parser.mb_width() || hdr->mb_height != s->parser.mb_height() || hdr->num_macroblocks != nmb )
    return fail( AA_ERR_ARGUMENT, "aa_stream_append_records: the header's macroblock dimensions are not this decoder's" );
  if ( hdr->num_coeff_blocks > nmb * 25 ) return fail( AA_ERR_ARGUMENT, "aa_stream_append_records: more coefficient blocks than macroblocks can hold" );
  // every macroblock's blocks must lie inside the array that came with it (the kernels trust coeff_index + popcount( nz_mask ))
  uint32_t intra = 0;
  for ( size_t i = 0; i < nmb; i++ ) {
    const uint32_t nblk = static_cast<uint32_t>( __builtin_popcount( mbs_in[i].nz_mask & 0x1FFFFFFu ) );
    if ( ( mbs_in[i].nz_mask >> 25 ) || ( nblk && size_t( mbs_in[i].coeff_index ) + nblk > hdr->num_coeff_blocks ) )
      return fail( AA_ERR_ARGUMENT, "aa_stream_append_records: macroblock " + std::to_string( i ) + " points outside the coefficient blocks" );
    if ( mbs_in[i].y_mode > 9 || mbs_in[i].uv_mode > 3 || mbs_in[i].ref_frame > 3 || mbs_in[i].segment_id > 3 || mbs_in[i].lf_level > 63 )
      return fail( AA_ERR_ARGUMENT, "aa_stream_append_records: macroblock " + std::to_string( i ) + " has a field out of range" );
    if ( !( mbs_in[i].flags & AA_MB_INTER ) ) intra++;
    else if ( hdr->key_frame ) return fail( AA_ERR_ARGUMENT, "aa_stream_append_records: inter macroblock in a key frame" );
  }
  return append_host_frame( s, frame_index, nullptr, [&]( aa_frame_header & h, aa_mb_info * mbs, int16_t * coeffs ) {
    h = *hdr;
    h.num_intra_mbs = intra; h.has_intra_mb = intra != 0;
    std::memcpy( mbs, mbs_in, nmb * sizeof( aa_mb_info ) );
    if ( hdr->num_coeff_blocks ) std::memcpy( coeffs, coeffs_in, size_t( hdr->num_coeff_blocks ) * 32 );
  } );
}

aa_status aa_stream_upload( aa_stream * s )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  bool any = false;
  for ( auto & c : s->chunks ) {
    if ( c.host && c.uploaded < c.used ) {
      HIP_TRY( hipMemcpyAsync( c.dev + c.uploaded, c.host + c.uploaded, c.used - c.uploaded, hipMemcpyHostToDevice, s->ctx->copy ) );
      c.uploaded = c.used; any = true;
    }
  }
  if ( any ) {
    HIP_TRY( hipEventRecord( s->ctx->upload_done, s->ctx->copy ) );
    HIP_TRY( hipStreamWaitEvent( s->ctx->compute, s->ctx->upload_done, 0 ) );
  }
  return AA_OK;
}

aa_status aa_stream_release_staging( aa_stream * s )
{
  if ( !s ) return fail( AA_ERR_ARGUMENT, "null stream" );
  if ( aa_status st = set_device( s->ctx ) ) return st;
  if ( aa_status st = aa_stream_upload( s ) ) return st;
  HIP_TRY( hipStreamSynchronize( s->ctx->copy ) );
  for ( auto & c : s->chunks ) {
    if ( !c.host ) continue;
    { std::lock_guard<std::mutex> g( s->ctx->pool_mu ); s->ctx->pinned_pool.emplace_back( c.host, c.pinned_bytes ); }
    c.host = nullptr;
    c.capacity = c.used;           // sealed: the next frame is staged in a new chunk
  }
  for ( auto & f : s->frames ) f.host_job = nullptr;
  return AA_OK;
}


/* ---------------- device-side entropy decode ---------------- */
namespace {
struct SubmitItem {
  aa_stream * s; const uint8_t * data; size_t size;
  size_t data_off;          // in the batch arena
  size_t rec_off = 0;       // the frame's record block, in the device half of the arena only
  aa_status status = AA_OK; std::string error;
  int frame_index = -1;
  bool seg_enabled = false, seg_reset = false;
  bool on_host = false;     // goes to a host lane (aa_ctx::HostLanes), not to the GPU's job queue
};

// one frame of one stream: header pre-pass on the host, compressed bytes into the pinned arena, record block + raster slot
aa_status submit_one( Batch * b, SubmitItem & it, int item, aa::ParseJob * jobs_host, aa_dev_frame * dframes_host, bool want_host_lane )
{
  aa_stream * s = it.s;
  aa_ctx * ctx = s->ctx;
  aa::ParseJob & J = jobs_host[item];
  FrameRec rec;
  try { s->parser.parse_header( it.data, it.size, rec.hdr, J.fp ); }
  catch ( const aa::ParseError & e ) { it.error = e.message; return e.code; }
  it.seg_enabled = J.fp.seg_enabled; it.seg_reset = s->parser.segment_map_reset();
  std::memcpy( b->host + it.data_off, it.data, it.size );

  const uint32_t nmb = uint32_t( J.fp.mbw ) * J.fp.mbh;
  const size_t mb_bytes = align_up( size_t( nmb ) * sizeof( aa_mb_info ) );
  const size_t words_per_row = ( J.fp.mbw + 63 ) / 64;
  const size_t rows_bytes = align_up( words_per_row * J.fp.mbh * sizeof( unsigned long long ) );
  const uint32_t flags_padded = ( nmb + 15u ) & ~15u;
  // one lane per partition: a second copy of the flags laid out partition by partition, a longer chunk list (tok_fsm.hh)
  const bool mp = ctx->tok.lane_per_partition && J.fp.nparts > 1;
  const uint32_t mp_stride = mp ? aa::mp_flag_stride( J.fp.mbw, J.fp.mbh, J.fp.nparts ) : 0u;
  const size_t flags_bytes = align_up( size_t( flags_padded ) + size_t( J.fp.nparts ) * mp_stride );
  const size_t list_bytes = align_up( size_t( aa::chunk_list_entries( nmb, mp ? J.fp.nparts : 1u ) ) * sizeof( uint32_t ) );

  const size_t pos_bytes = ctx->tok.packed ? align_up( size_t( nmb ) * sizeof( uint32_t ) ) : 0;
  rec.rec_bytes = mb_bytes + rows_bytes + flags_bytes + list_bytes + pos_bytes;
  rec.rec_block = b->dev + it.rec_off; rec.rec_in_arena = true;
  uint8_t * blk = rec.rec_block;

  J.data = b->dev + it.data_off;
  J.size = static_cast<uint32_t>( it.size ); J.data_padded = ( J.size + 15u ) & ~15u;
  J.nmb = nmb; J.flags_padded = flags_padded; J.mp_stride = mp_stride; J.mp_pad = 0;
  J.mbs = reinterpret_cast<aa_mb_info *>( blk );
  J.intra_rows = reinterpret_cast<unsigned long long *>( blk + mb_bytes );
  J.mbflags = blk + mb_bytes + rows_bytes;
  J.chunk_list = reinterpret_cast<uint32_t *>( blk + mb_bytes + rows_bytes + flags_bytes );
  J.packed_pos = pos_bytes ? reinterpret_cast<uint32_t *>( blk + mb_bytes + rows_bytes + flags_bytes + list_bytes ) : nullptr;
  rec.packed_pos = J.packed_pos; rec.dev_mbs = J.mbs;
  J.summary = reinterpret_cast<aa::FrameSummary *>( b->host_dev + b->summaries_off ) + item;     // pinned + mapped: no copy back
  rec.chunk_list = J.chunk_list;
  rec.summary = reinterpret_cast<volatile aa::FrameSummary *>( b->host + b->summaries_off ) + item;
  rec.parse_job = reinterpret_cast<const aa::ParseJob *>( b->dev ) + item;

  aa_dev_frame * job = &dframes_host[item];
  rec.hdr.has_intra_mb = 1;              // until the device parser has counted: the row masks say which macroblocks are intra
  fill_job( rec, job );
  job->mbs = J.mbs; job->intra_rows = J.intra_rows;
  job->coeffs = reinterpret_cast<const int16_t *>( ctx->tok.heap );     // coeff_index of a device-parsed macroblock = its first block's index in the heap
  job->packed = ctx->tok.packed ? 1u : 0u;                              // ... packed storage: the 40-bit offset of its words (tok_fsm.hh store_mb_packed)
  rec.host_job = job;
  rec.dev_job = reinterpret_cast<const aa_dev_frame *>( b->dev + ( reinterpret_cast<uint8_t *>( job ) - b->host ) );
  rec.batch = b; rec.batch_item = item; rec.summary_pending = true;
  if ( want_host_lane && !J.fp.seg_enabled ) {
    // A host lane takes the frame (not one of a stream that uses segmentation: the persistent segment map is the one piece of
    // macroblock data a frame inherits, and that stream's map lives on the device).  Its records are dense blocks in a piece of
    // their own, like a host-parsed frame's: no chunk list, no packed words; and it counts as handed over from now on -- whoever
    // releases it waits for the worker's `done` word.
    it.on_host = true;
    job->packed = 0;
    rec.packed_pos = nullptr; rec.chunk_list = nullptr;
    rec.enqueued = true;
  }
  it.frame_index = static_cast<int>( s->frames.size() );
  s->frames.push_back( std::move( rec ) );
  return AA_OK;
}
} // namespace

namespace {
// second phase of a batch: its frames go to the job queue of the token workers (behind the macroblock-header kernel on the
// batch's stream), the heap is grown for what they are expected to store, workgroups are launched if too few are alive
aa_status launch_tokens_of( aa_ctx * ctx, Batch * b )
{
  if ( !b->tokens_pending ) return AA_OK;
  auto & T = ctx->tok;
  aa::ParseJob * jobs_host = reinterpret_cast<aa::ParseJob *>( b->host );
  // the ring of job slots must not wrap onto jobs that have not been taken
  if ( static_cast<uint32_t>( T.jobs_enqueued ) - T.mirror_host->q_head + static_cast<uint32_t>( b->n ) + 4096u > T.q_slots ) {
    if ( aa_status st = tok_refresh_mirror( ctx ) ) return st;
    if ( static_cast<uint32_t>( T.jobs_enqueued ) - T.mirror_host->q_head + static_cast<uint32_t>( b->n ) + 4096u > T.q_slots )
      if ( aa_status st = tok_quiesce( ctx ) ) return st;
  }
  b->tokens_pending = false;
  ctx->deferred.erase( std::remove( ctx->deferred.begin(), ctx->deferred.end(), b ), ctx->deferred.end() );
  bool dropped = false;
  tok_prune_inflight( ctx );
  for ( int i = 0; i < b->n; i++ ) {
    Batch::Item & it = b->items[i];
    if ( !it.live ) { if ( jobs_host[i].nmb ) { jobs_host[i].nmb = 0; dropped = true; } continue; }   // rejected by the pre-pass, or released since: the lane that draws it drops it
    FrameRec & r = it.s->frames[it.frame];
    if ( it.on_host ) continue;                    // (a host lane's: no ticket, no chunks)
    r.enqueued = true;
    // what the frame is expected to store, in chunks: blocks per compressed byte as frames have turned out so far (the ratio
    // holds across key and inter frames and quantisers far better than blocks per macroblock), a margin, and the chunk its
    // lane will be filling when it ends
    if ( T.packed ) {
      const double words = std::min( double( aa::kMbWords ) * jobs_host[i].nmb, T.words_per_byte * 1.15 * jobs_host[i].size );
      r.est_chunks = static_cast<uint32_t>( words / ( aa::kChunkWords - aa::kMbWords ) ) + 1u;
    } else {
      const double blocks = std::min( 25.0 * jobs_host[i].nmb, T.blocks_per_byte * 1.15 * jobs_host[i].size );
      r.est_chunks = static_cast<uint32_t>( blocks / ( aa::kChunkBlocks - aa::kMbBlocks ) ) + 1u;
    }
    // (one lane per partition: every lane of the frame fills a chunk of its own -- P - 1 more partly filled chunks than the words say;
    // without them the heap was mapped for a quarter of what 4-partition frames take and their lanes sat out the 2-s memory wait)
    if ( T.lane_per_partition && jobs_host[i].mp_stride && jobs_host[i].fp.nparts > 1 ) r.est_chunks += static_cast<uint32_t>( jobs_host[i].fp.nparts ) - 1u;
    T.chunks_committed += r.est_chunks;
    ctx->stats.parsed_macroblocks += jobs_host[i].nmb;
  }
  if ( std::find( T.inflight.begin(), T.inflight.end(), b ) == T.inflight.end() ) T.inflight.push_back( b );
  if ( std::find( T.batches.begin(), T.batches.end(), b ) == T.batches.end() ) T.batches.push_back( b );
  if ( aa_status st = tok_grow_heap( ctx, static_cast<size_t>( std::max<int64_t>( 0, T.chunks_committed ) ) * kChunkBytesHeap ) ) return st;
  hipStream_t ps = b->ps;
  if ( b->patch_jobs && dropped ) HIP_TRY( hipMemcpyAsync( b->dev, b->host, b->head_bytes, hipMemcpyHostToDevice, ps ) );     // (behind the header kernel on its stream)
  if ( dropped ) {
    // frames released between the two phases of a two-phase submit get no ticket: release_records waits only for frames that
    // were handed to the queue, so a ticket nobody waits for could be drawn after the arena has been recycled
    int keep = 0;
    for ( int k = 0; k < b->n_order; k++ ) if ( b->items[b->launch_order_host[k]].live ) b->launch_order_host[keep++] = b->launch_order_host[k];
    b->n_order = keep;
    if ( keep ) HIP_TRY( hipMemcpyAsync( const_cast<uint32_t *>( b->launch_order_dev ), b->launch_order_host, size_t( keep ) * sizeof( uint32_t ), hipMemcpyHostToDevice, ps ) );
  }
  if ( b->n_order > 0 ) {
    if ( int e = aa::launch_enqueue_jobs( T.q, T.slots, reinterpret_cast<const aa::ParseJob *>( b->dev ), b->launch_order_dev, b->n_order, ps ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_enqueue_jobs" );
    T.jobs_enqueued += static_cast<uint64_t>( b->n_order );
  }
  HIP_TRY( hipEventRecord( b->hdr_done, ps ) );
  HIP_TRY( hipEventRecord( ctx->parse_idle[b->parse_stream_index], ps ) );
  return tok_service( ctx, b->hdr_done );
}
} // namespace

namespace {
// ---- host lanes (aa_ctx::HostLanes) ----
// One frame: macroblock headers + tokens from the arena's pinned copy (the header pre-pass left everything else in its ParseJob),
// records to HBM where the frame's job record says they are, dense coefficient blocks to a pool piece of their own, then the
// summary and -- last, behind the copies -- the `done` word.  Scratch buffers are the worker's own, kept from frame to frame.
// (PINNED: a copy out of pageable memory makes the runtime pin and unpin pages under every transfer -- page-table updates that hold up
// the whole GPU; with sixteen workers uploading 5-MB key frames that was enough to run a row kernel's bounded wait out during priming)
struct HostLaneScratch {
  uint8_t * pin = nullptr; size_t pin_bytes = 0;      // macroblock records | intra row masks | worst-case dense coefficient blocks
  std::vector<uint8_t> above; hipEvent_t ev = nullptr;
  bool fit( size_t bytes )
  {
    if ( bytes <= pin_bytes ) return true;
    if ( pin ) (void) hipHostFree( pin );
    pin = nullptr; pin_bytes = 0;
    if ( hipHostMalloc( reinterpret_cast<void **>( &pin ), bytes, hipHostMallocDefault ) != hipSuccess ) { (void) hipGetLastError(); pin = nullptr; return false; }
    pin_bytes = bytes;
    return true;
  }
};
void host_lane_run( aa_ctx * ctx, Batch * b, int item, HostLaneScratch & S )
{
  const aa::ParseJob & J = reinterpret_cast<const aa::ParseJob *>( b->host )[item];
  volatile aa::FrameSummary * sum = reinterpret_cast<volatile aa::FrameSummary *>( b->host + b->summaries_off ) + item;
  Batch::Item & it = b->items[item];
  const uint32_t mbw = J.fp.mbw, mbh = J.fp.mbh, nmb = mbw * mbh;
  const size_t words_per_row = ( mbw + 63 ) / 64;
  uint32_t status = aa::TOK_OK, blocks = 0, intra = 0, split = 0;
  hipStream_t up = ctx->tok.host_up;              // (behind the arena's upload: the submit call made this stream wait for it)
  if ( !S.ev ) status = aa::TOK_HOST_FAILED;      // (no event to wait for the uploads with: see host_lanes_main)
  const size_t mbs_bytes = align_up( size_t( nmb ) * sizeof( aa_mb_info ) ), rows_bytes = align_up( words_per_row * mbh * sizeof( unsigned long long ) );
  try { S.above.resize( size_t( mbw ) * 9 ); } catch ( const std::bad_alloc & ) { status = aa::TOK_HOST_FAILED; }
  if ( status == aa::TOK_OK && !S.fit( mbs_bytes + rows_bytes + size_t( nmb ) * 25 * 32 + 256 ) ) status = aa::TOK_HOST_FAILED;
  if ( status == aa::TOK_OK ) {
    aa_mb_info * mbs = reinterpret_cast<aa_mb_info *>( S.pin );
    unsigned long long * rows = reinterpret_cast<unsigned long long *>( S.pin + mbs_bytes );
    int16_t * coeffs = reinterpret_cast<int16_t *>( S.pin + mbs_bytes + rows_bytes );
    std::memset( static_cast<void *>( mbs ), 0, size_t( nmb ) * sizeof( aa_mb_info ) );
    const double t_parse = now_ms();
    aa::parse_frame_body( b->host + it.data_off, J.fp, mbs, coeffs, S.above.data(), &blocks, &intra );
    ctx->host_lanes.parse_us += static_cast<uint64_t>( ( now_ms() - t_parse ) * 1e3 ); ctx->host_lanes.parsed_bytes += J.size;
    std::memset( rows, 0, words_per_row * mbh * sizeof( unsigned long long ) );
    for ( uint32_t r = 0; r < mbh; r++ ) for ( uint32_t c = 0; c < mbw; c++ ) {
      const aa_mb_info & mb = mbs[r * mbw + c];
      if ( !( mb.flags & AA_MB_INTER ) ) rows[r * words_per_row + ( c >> 6 )] |= 1ull << ( c & 63 );
      else if ( mb.y_mode == aa::SPLITMV ) split = 1;
    }
    uint8_t * dense = nullptr;
    const size_t dense_bytes = align_up( std::max<size_t>( size_t( blocks ) * 32, 32 ) );
    hipError_t e = hipSuccess;
    if ( dev_alloc( ctx, dense_bytes, &dense ) != AA_OK ) status = aa::TOK_HOST_FAILED;
    else {
      it.host_dense = dense; it.host_dense_bytes = dense_bytes;
      // (the arena's upload -- which carries the job record as the pre-pass left it -- was queued on the copy stream by the submit call,
      // which also made the host lanes' stream wait for it)
      e = hipMemcpyAsync( J.mbs, mbs, size_t( nmb ) * sizeof( aa_mb_info ), hipMemcpyHostToDevice, up );
      if ( e == hipSuccess ) e = hipMemcpyAsync( J.intra_rows, rows, words_per_row * mbh * sizeof( unsigned long long ), hipMemcpyHostToDevice, up );
      if ( e == hipSuccess && blocks ) e = hipMemcpyAsync( dense, coeffs, size_t( blocks ) * 32, hipMemcpyHostToDevice, up );
      if ( e == hipSuccess ) {
        // the frame's reconstruction job record (aa_dev_frame, in the arena behind the parse jobs): its blocks are here, not in the heap
        uint8_t * job_dev = b->dev + align_up( size_t( b->n ) * sizeof( aa::ParseJob ) ) + size_t( item ) * sizeof( aa_dev_frame );
        const int16_t ** dense_ptr = reinterpret_cast<const int16_t **>( S.pin + S.pin_bytes - 16 );       // (pinned too: the last bytes of the scratch)
        *dense_ptr = reinterpret_cast<const int16_t *>( dense );
        e = hipMemcpyAsync( job_dev + offsetof( aa_dev_frame, coeffs ), dense_ptr, sizeof *dense_ptr, hipMemcpyHostToDevice, up );
      }
      if ( e == hipSuccess ) e = hipEventRecord( S.ev, up );
      if ( e == hipSuccess ) e = hipEventSynchronize( S.ev );
      if ( e != hipSuccess ) status = aa::TOK_HOST_FAILED;
    }
  }
  sum->num_coeff_blocks = blocks; sum->num_intra_mbs = intra; sum->has_split = split; sum->steps = 0; sum->num_chunks = 0; sum->packed_words = 0;
  sum->status = status;
  ctx->host_lanes.backlog_bytes -= J.size;
  __atomic_thread_fence( __ATOMIC_RELEASE );
  sum->done = 1u;
}
void host_lanes_main( aa_ctx * ctx )
{
  (void) hipSetDevice( ctx->device );
  HostLaneScratch S;
  for ( int tries = 0; tries < 3 && !S.ev; tries++ )     // (without it the worker can only fail its frames: host_lane_run says TOK_HOST_FAILED)
    if ( hipEventCreateWithFlags( &S.ev, hipEventDisableTiming ) != hipSuccess ) { (void) hipGetLastError(); S.ev = nullptr; usleep( 1000 ); }
  auto & H = ctx->host_lanes;
  for ( ;; ) {
    aa_ctx::HostLanes::Task t;
    {
      std::unique_lock<std::mutex> g( H.mu );
      H.cv.wait( g, [&] { return H.stop || !H.q.empty(); } );
      if ( H.q.empty() ) break;                      // (stop: after the queue has been worked off -- somebody may wait for those frames)
      t = H.q.front(); H.q.pop_front();
    }
    host_lane_run( ctx, t.b, t.item, S );
  }
  if ( S.ev ) (void) hipEventDestroy( S.ev );
  if ( S.pin ) (void) hipHostFree( S.pin );
}
void host_lanes_start( aa_ctx * ctx )
{
  auto & H = ctx->host_lanes;
  if ( !H.threads.empty() ) return;
  int nt = effective_cpus();
  if ( const char * e = std::getenv( "ALFALFA_AMD_HOST_LANES" ) ) nt = std::max( 1, atoi( e ) );
  for ( int t = 0; t < nt; t++ ) H.threads.emplace_back( host_lanes_main, ctx );
}
// compressed bytes the host lanes get through per millisecond, all workers together (measured on the frames parsed so far --
// parse time only, so a cold first call's allocations do not depress it; before the first frame: 24 KB/ms per usable core)
double host_lanes_rate( aa_ctx * ctx )
{
  auto & H = ctx->host_lanes;
  int nt = static_cast<int>( H.threads.size() );
  if ( !nt ) { nt = effective_cpus(); if ( const char * e = std::getenv( "ALFALFA_AMD_HOST_LANES" ) ) nt = std::max( 1, atoi( e ) ); }
  const uint64_t us = H.parse_us.load(), bytes = H.parsed_bytes.load();
  const double per_worker = us > 1000 ? static_cast<double>( bytes ) / static_cast<double>( us ) * 1e3 : 24.0e3;     // bytes per ms
  return per_worker * std::min( nt, effective_cpus() );
}
void host_lanes_stop( aa_ctx * ctx )
{
  auto & H = ctx->host_lanes;
  { std::lock_guard<std::mutex> g( H.mu ); H.stop = true; }
  H.cv.notify_all();
  for ( auto & t : H.threads ) t.join();
  H.threads.clear();
}
} // namespace

aa_status aa_launch_tokens( aa_ctx * ctx, int max_batches, int * launched_out )
{
  if ( !ctx ) return fail( AA_ERR_ARGUMENT, "aa_launch_tokens: null context" );
  if ( aa_status st = set_device( ctx ) ) return st;
  int launched = 0;
  while ( !ctx->deferred.empty() && ( max_batches <= 0 || launched < max_batches ) ) {
    if ( aa_status st = launch_tokens_of( ctx, ctx->deferred.front() ) ) return st;
    launched++;
  }
  if ( launched_out ) *launched_out = launched;
  return AA_OK;
}

aa_status aa_submit_frames( aa_ctx * ctx, const aa_frame_in * frames, int n, int * frame_index_out, int threads )
{
  return aa_submit_frames_ex( ctx, frames, n, frame_index_out, threads, 0 );
}

aa_status aa_submit_frames_ex( aa_ctx * ctx, const aa_frame_in * frames, int n, int * frame_index_out, int threads, unsigned flags )
{
  if ( !ctx || !frames || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_submit_frames: bad argument" );
  const bool defer_tokens = ( flags & AA_SUBMIT_DEFER_TOKENS ) != 0;
  if ( aa_status st = set_device( ctx ) ) return st;
  if ( aa_status st = tok_init( ctx ) ) return st;
  std::vector<SubmitItem> items( n );
  // arena layout: parse jobs | reconstruction job records | summaries | segment-pass lists | compressed frames
  const size_t jobs_bytes = align_up( size_t( n ) * sizeof( aa::ParseJob ) );
  const size_t dframes_bytes = align_up( size_t( n ) * sizeof( aa_dev_frame ) );
  const size_t sums_bytes = align_up( size_t( n ) * sizeof( aa::FrameSummary ) );
  const size_t seg_bytes = align_up( size_t( n ) * ( sizeof( aa_seg_stream ) + 2 * sizeof( uint32_t ) ) );   // + the launch order
  size_t off = jobs_bytes + dframes_bytes + sums_bytes + seg_bytes;
  std::map<aa_stream *, std::vector<int>> by_stream;
  std::vector<aa_stream *> stream_order;
  for ( int i = 0; i < n; i++ ) {
    if ( !frames[i].stream || !frames[i].data || frames[i].stream->ctx != ctx ) return fail( AA_ERR_ARGUMENT, "aa_submit_frames: null frame or stream of another context" );
    items[i].s = frames[i].stream; items[i].data = frames[i].data; items[i].size = frames[i].size;
    items[i].data_off = off;
    off += align_up( frames[i].size + 16 );
    auto & v = by_stream[frames[i].stream];
    if ( v.empty() ) stream_order.push_back( frames[i].stream );
    v.push_back( i );
  }
  for ( aa_stream * s : stream_order )
    if ( s->next_submit > static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_LOGIC, "aa_submit_frames: stream state is inconsistent" );

  bool to_host_lanes = false;
  std::vector<char> host_lane_wanted( n, 0 );     // [i]: frame i should go to a host lane (if it may: submit_one)
  // ---- route: few chains -> the host's cores ----
  // A GPU lane decodes a bool in ~0.3 us, a host core in ~4 ns: one core is worth ~75 lanes, and a frame on a lane is a chain of
  // seconds whatever else the GPU does.  The GPU wins by holding 22 000 chains at once; a call with fewer streams than the host
  // has workers (an ExCamera bundle of 8 chunks, a player's single stream) is through sooner -- and at a higher rate -- when
  // each stream's frames are parsed by one host worker (Parser::parse, the same records) and uploaded.  Frames of one stream
  // are serial on a core, so what counts is streams per worker, not frames.
  {
    const int nt = worker_threads( threads );
    const char * route_env = std::getenv( "ALFALFA_AMD_ROUTE" );            // "device" / "host": tests and experiments; default: by size
    const bool force_device = ( flags & AA_SUBMIT_DEVICE ) || ( route_env && route_env[0] == 'd' );
    const bool force_host = ( flags & AA_SUBMIT_HOST ) || ( route_env && route_env[0] == 'h' );
    // measured (round 3, 1080p, 256-core host): 1 stream 0.67 M macroblocks/s on the host route vs 0.14 M on the GPU lanes, 8 streams
    // 4.8 M vs 2.4 M -- but 64 streams 9.8 M vs 14.9 M (64 workers do not scale on this host's memory system): the bound is 24
    const bool few = static_cast<int>( stream_order.size() ) <= std::min( nt, 24 );
    if ( !defer_tokens && !force_device && force_host && !few ) {
      // many streams, and the caller wants them parsed by the host's cores (AA_SUBMIT_HOST: frames that are needed at once -- the key
      // frames of the group a pipeline starts with: 35 ms on a core, 2 s as a chain on a lane): HOST LANES.  The frames take the
      // device route below -- header pre-pass, arena, records in HBM -- but their tickets go to worker threads of the context, which
      // finish them with the `done` word a GPU lane writes.  The call does not wait for them (round 4's version of this route did,
      // ~1 s for a group's key frames, and the hand-overs behind it started that much later).
      to_host_lanes = true;
    }
    // Round 6: FRAME-PARALLEL parse of few streams.  A call that brings SEVERAL frames per stream (a player's look-ahead, an ExCamera
    // bundle's chunks: player.cc:134-144, decode-bundle.cc:56-99) used to parse each stream's frames one after the other on one
    // worker -- one stream = one core, whatever the box has -- and inside the call.  VP8 has no backward adaptation: once the header
    // pre-pass (microseconds per frame, serial across a stream) has run, every frame body is an independent chain
    // (decoder_state.hh:92-97,126-131), which is exactly what the host lanes take.  Such a call therefore goes the host lanes' way
    // too: all its frames in parallel on the context's worker threads, the call returns at once, reconstruction waits for each
    // frame's `done` word.  Not for streams that use segmentation (their persistent map lives with whoever parses them in order:
    // the per-stream route below) and not for one-frame-per-stream calls (nothing to run in parallel; the caller waits anyway).
    if ( !defer_tokens && !force_device && !force_host && few && !to_host_lanes && n > static_cast<int>( stream_order.size() ) ) {
      const char * few_env = std::getenv( "ALFALFA_AMD_FEW_ROUTE" );
      const bool per_stream = few_env && few_env[0] == 's';                // "streams": the round-3 route (A/B runs, tests)
      bool seg = false;
      for ( aa_stream * s : stream_order ) seg = seg || s->parser.segmentation().enabled || s->segmap_on_device;
      if ( !per_stream && !seg ) to_host_lanes = true;
    }
    if ( !defer_tokens && !force_device && !to_host_lanes && ( force_host || few ) ) {
      std::atomic<size_t> next { 0 };
      auto work = [&]() {
        for ( ;; ) {
          const size_t k = next.fetch_add( 1 );
          if ( k >= stream_order.size() ) return;
          bool broken = false;
          for ( int i : by_stream[stream_order[k]] ) {
            SubmitItem & it = items[i];
            if ( broken ) { it.status = AA_ERR_LOGIC; it.error = "an earlier frame of this stream in the same call failed"; continue; }
            it.status = aa_stream_parse( it.s, it.data, it.size, &it.frame_index, nullptr );
            if ( it.status != AA_OK ) { it.error = g_last_error; it.frame_index = -1; broken = true; }
          }
        }
      };
      const int workers = std::max( 1, std::min<int>( nt, static_cast<int>( stream_order.size() ) ) );
      if ( workers == 1 ) work();
      else {
        std::vector<std::thread> pool;
        for ( int t = 0; t < workers; t++ ) pool.emplace_back( work );
        for ( auto & t : pool ) t.join();
      }
      ctx->stats.host_routed_frames += static_cast<uint64_t>( n );
      aa_status first_error = AA_OK; std::string first_message;
      for ( int i = 0; i < n; i++ ) {
        if ( frame_index_out ) frame_index_out[i] = items[i].frame_index;
        if ( items[i].status != AA_OK && first_error == AA_OK ) { first_error = items[i].status; first_message = items[i].error; }
      }
      return first_error == AA_OK ? AA_OK : fail( first_error, first_message );
    }
    // ---- hybrid: a big call's KEY frames on the host's cores, the rest on the lanes ----
    // A key frame's chain is the longest there is (2.2 s on a lane at 1080p, ~35 ms on a core) and nothing of its group can be
    // reconstructed before it is parsed; a call's key frames are few (one per stream and group of pictures).  Streams whose
    // frames in this call are all key frames go to the HOST LANES, biggest first, while what the host lanes have been given and
    // not finished stays within `host_share_ms` of their work (at the rate they have really achieved: bytes of compressed frames
    // per millisecond of a worker's parse time x workers; until measured, 24 KB/ms per usable core); everything else takes the
    // GPU's lanes.  Nothing here waits: round 4's version of this share parsed inside the call and was worth taking only when
    // the host could have half of a call's key frames within the budget.
    if ( !defer_tokens && !force_device && !to_host_lanes && ctx->host_share_ms > 0 ) {
      std::vector<std::pair<size_t, aa_stream *>> cand;
      for ( aa_stream * s : stream_order ) {
        size_t bytes = 0; bool all_key = true;
        for ( int i : by_stream[s] ) { all_key = all_key && frames[i].size >= 10 && ( frames[i].data[0] & 1u ) == 0u; bytes += frames[i].size; }
        if ( all_key ) cand.emplace_back( bytes, s );
      }
      std::stable_sort( cand.begin(), cand.end(), []( const auto & a, const auto & b ) { return a.first > b.first; } );
      const double capacity_bytes = ctx->host_share_ms * host_lanes_rate( ctx );
      double taken = static_cast<double>( ctx->host_lanes.backlog_bytes.load() );
      for ( auto & c : cand ) {
        if ( taken + static_cast<double>( c.first ) > capacity_bytes ) break;
        taken += static_cast<double>( c.first );
        for ( int i : by_stream[c.second] ) host_lane_wanted[i] = 1;
      }
    }
  }
  if ( to_host_lanes ) std::fill( host_lane_wanted.begin(), host_lane_wanted.end(), 1 );

  std::unique_ptr<Batch> b( new Batch );
  const size_t arena = ( off + ( size_t( 16 ) << 20 ) - 1 ) & ~( ( size_t( 16 ) << 20 ) - 1 );
  // The frames' record blocks (macroblock records, flags, chunk list: written by the parse kernels only) sit behind the mirrored
  // part in the DEVICE half of the arena: one piece of the pool per call instead of one per frame (thousands of allocator
  // round trips per call); they go back when the last frame of the call is released.
  size_t dev_arena = arena;
  for ( int i = 0; i < n; i++ ) {
    const aa_stream * s = frames[i].stream;
    const size_t nmb = size_t( s->parser.mb_width() ) * s->parser.mb_height();
    const size_t words_per_row = ( s->parser.mb_width() + 63 ) / 64;
    items[i].rec_off = dev_arena;
    dev_arena += align_up( nmb * sizeof( aa_mb_info ) ) + align_up( words_per_row * s->parser.mb_height() * sizeof( unsigned long long ) )
                 + ( ctx->tok.lane_per_partition      // (how many partitions a frame has is known after its pre-pass: room for 8)
                       ? align_up( ( ( nmb + 15u ) & ~size_t( 15 ) ) + 8 * size_t( aa::mp_flag_stride( s->parser.mb_width(), s->parser.mb_height(), 8 ) ) )
                         + align_up( size_t( aa::chunk_list_entries( static_cast<uint32_t>( nmb ), 8 ) ) * sizeof( uint32_t ) )
                       : align_up( ( nmb + 15u ) & ~size_t( 15 ) ) + align_up( size_t( aa::chunk_list_entries( static_cast<uint32_t>( nmb ) ) ) * sizeof( uint32_t ) ) )
                 + ( ctx->tok.packed ? align_up( nmb * sizeof( uint32_t ) ) : 0 );
  }
  dev_arena = ( dev_arena + ( size_t( 16 ) << 20 ) - 1 ) & ~( ( size_t( 16 ) << 20 ) - 1 );
  b->host = pinned_get( ctx, arena, &b->host_bytes );
  if ( !b->host ) return fail( AA_ERR_HIP, "aa_submit_frames: pinned staging allocation failed" );
  b->dev_bytes = dev_arena;
  if ( aa_status st = dev_alloc( ctx, dev_arena, &b->dev, true ) ) { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->pinned_pool.emplace_back( b->host, b->host_bytes ); return st; }
  b->n = n; b->summaries_off = jobs_bytes + dframes_bytes;
  if ( hipError_t e = hipHostGetDevicePointer( reinterpret_cast<void **>( &b->host_dev ), b->host, 0 ) ) {
    { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->pinned_pool.emplace_back( b->host, b->host_bytes ); }
    dev_free( ctx, b->dev, b->dev_bytes );
    return hip_fail( e, "hipHostGetDevicePointer (batch arena)" );
  }
  aa::ParseJob * jobs_host = reinterpret_cast<aa::ParseJob *>( b->host );
  aa_dev_frame * dframes_host = reinterpret_cast<aa_dev_frame *>( b->host + jobs_bytes );
  std::memset( b->host, 0, jobs_bytes + dframes_bytes + sums_bytes + seg_bytes );

  // ---- host half, one worker per stream at a time (the header pre-pass is serial across the frames of a stream) ----
  {
    std::atomic<size_t> next { 0 };
    // (while the host lanes have frames to parse -- frames somebody needs at once -- the pre-pass workers of later hand-overs step
    // back: a thread may lower its own priority.  On a box that grants 16 CPUs the first group's key frames were seen to take 4 s
    // instead of 1 when twenty hand-overs' worth of pre-pass threads and arena copies ran beside them.)
    const int nt = std::min<int>( worker_threads( threads ), static_cast<int>( stream_order.size() ) );
    const bool step_back = nt > 1 && ctx->host_lanes.backlog_bytes.load() > 0;          // (nt == 1: the caller's own thread does the work)
    auto work = [&]() {
      (void) hipSetDevice( ctx->device );
      if ( step_back ) (void) setpriority( PRIO_PROCESS, static_cast<id_t>( syscall( SYS_gettid ) ), 10 );
      for ( ;; ) {
        const size_t k = next.fetch_add( 1 );
        if ( k >= stream_order.size() ) return;
        bool broken = false;
        for ( int i : by_stream[stream_order[k]] ) {
          SubmitItem & it = items[i];
          if ( broken ) { it.status = AA_ERR_LOGIC; it.error = "an earlier frame of this stream in the same call failed"; continue; }
          it.status = submit_one( b.get(), it, i, jobs_host, dframes_host, host_lane_wanted[i] != 0 );
          if ( it.status != AA_OK ) broken = true;
        }
      }
    };
    if ( nt == 1 ) work();
    else {
      std::vector<std::thread> pool;
      for ( int t = 0; t < nt; t++ ) pool.emplace_back( work );
      for ( auto & t : pool ) t.join();
    }
  }
  aa_status first_error = AA_OK; std::string first_message;
  int appended = 0, max_mbw = 0, max_nparts = 1;
  for ( int i = 0; i < n; i++ ) {
    if ( frame_index_out ) frame_index_out[i] = items[i].frame_index;
    if ( items[i].status == AA_OK ) { appended++; max_mbw = std::max<int>( max_mbw, jobs_host[i].fp.mbw ); max_nparts = std::max<int>( max_nparts, jobs_host[i].fp.nparts ); }
    else {
      jobs_host[i].nmb = 0;                        // the kernels skip it
      if ( first_error == AA_OK ) { first_error = items[i].status; first_message = items[i].error; }
    }
  }
  if ( !appended ) {
    { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->pinned_pool.emplace_back( b->host, b->host_bytes ); }
    dev_free( ctx, b->dev, b->dev_bytes );
    return fail( first_error, first_message );
  }
  b->live = appended;
  b->items.resize( n );
  for ( int i = 0; i < n; i++ ) { b->items[i] = { items[i].s, items[i].frame_index, items[i].status == AA_OK }; b->items[i].on_host = items[i].status == AA_OK && items[i].on_host; b->items[i].data_off = items[i].data_off; }
  b->head_bytes = jobs_bytes + dframes_bytes;
  b->max_mbw = max_mbw; b->max_nparts = max_nparts;
  if ( ctx->tok.lane_per_partition ) ctx->tok.mp_hint = std::max<uint32_t>( ctx->tok.mp_hint, static_cast<uint32_t>( max_nparts ) );   // (workgroups launched from now on leave that many lanes per ticket)
  // From here on the frames that were appended point at the batch.  If anything below fails they are given back one by one
  // (the last one frees the batch): no frame is left with a dangling batch, nothing leaks; the frames themselves stay in
  // their streams as frames whose records are gone (decoding them reports that).
  struct Abandon {
    aa_ctx * ctx; Batch * b; bool armed = true;
    ~Abandon() {
      if ( !armed ) return;
      const std::string keep = g_last_error;
      {                                                     // (host lanes' frames that no worker was given: nobody will write their `done` word)
        volatile aa::FrameSummary * sums = reinterpret_cast<volatile aa::FrameSummary *>( b->host + b->summaries_off );
        for ( size_t i = 0; i < b->items.size(); i++ ) if ( b->items[i].on_host ) { sums[i].status = aa::TOK_HOST_FAILED; sums[i].done = 1u; }
      }
      std::vector<Batch::Item> its = b->items;              // (the batch dies with its last frame)
      for ( auto & it : its ) if ( it.live ) release_records( it.s, it.s->frames[it.frame], true );
      g_last_error = keep;
    }
  } abandon { ctx, b.release() };
  Batch * const raw = abandon.b;
  if ( aa_status st = tok_set_lane_bytes( ctx, aa::tok::lane_lds_bytes( static_cast<uint32_t>( max_mbw ), max_nparts > 1, ctx->tok.lane_per_partition ) ) ) return st;

  // ---- segment-map pass lists (only streams that use segmentation in this batch) ----
  aa_seg_stream * seg_streams = reinterpret_cast<aa_seg_stream *>( raw->host + jobs_bytes + dframes_bytes + sums_bytes );
  uint32_t * seg_order = reinterpret_cast<uint32_t *>( seg_streams + n );
  int n_seg_streams = 0; uint32_t n_seg_order = 0;
  // a stream with nothing queued if there is one (else the next in turn: the batch waits behind that stream's work)
  int pick = ctx->next_parse_stream;
  for ( int k = 0; k < ctx->n_parse_streams; k++ ) {
    const int c = ( ctx->next_parse_stream + k ) % ctx->n_parse_streams;
    if ( hipEventQuery( ctx->parse_idle[c] ) == hipSuccess ) { pick = c; break; }
  }
  (void) hipGetLastError();
  ctx->next_parse_stream = ( pick + 1 ) % ctx->n_parse_streams;
  raw->parse_stream_index = pick;
  hipStream_t ps = ctx->parse_streams[pick];
  for ( aa_stream * s : stream_order ) {
    bool any = false;
    for ( int i : by_stream[s] ) if ( items[i].status == AA_OK && items[i].seg_enabled ) any = true;
    if ( !any && !s->segmap_on_device ) continue;
    if ( !any ) continue;
    const size_t map_bytes = size_t( s->parser.mb_width() ) * s->parser.mb_height();
    if ( !s->dev_segmap ) if ( aa_status st = dev_alloc( ctx, map_bytes, &s->dev_segmap ) ) return st;
    if ( !s->segmap_on_device ) {                  // the host parser owns the current map: hand it over
      HIP_TRY( hipMemcpyAsync( s->dev_segmap, s->parser.segment_map().data(), map_bytes, hipMemcpyHostToDevice, ps ) );
      HIP_TRY( hipStreamSynchronize( ps ) );
      s->segmap_on_device = true;
    }
    aa_seg_stream & ss = seg_streams[n_seg_streams++];
    ss.map = s->dev_segmap; ss.first = n_seg_order; ss.count = 0;
    for ( int i : by_stream[s] ) if ( items[i].status == AA_OK ) { seg_order[n_seg_order++] = static_cast<uint32_t>( i ) | ( items[i].seg_reset ? 0x80000000u : 0u ); ss.count++; }
  }

  // launch order: longest chains first (the compressed size is the length of a token chain, near enough), so that the lanes
  // of a wave finish together and the long waves start first
  // (only frames the pre-pass accepted: a ticket in the job queue is a pointer into this arena that a lane may follow long
  // after the call -- a rejected frame has nobody who would wait for its lane before the arena is recycled)
  uint32_t * launch_order = seg_order + n;
  int n_order = 0;
  for ( int i = 0; i < n; i++ ) if ( items[i].status == AA_OK && !items[i].on_host ) launch_order[n_order++] = static_cast<uint32_t>( i );      // (host lanes' frames: no ticket)
  std::stable_sort( launch_order, launch_order + n_order, [&]( uint32_t a, uint32_t b ) { return items[a].size > items[b].size; } );
  const uint32_t * launch_order_dev = reinterpret_cast<const uint32_t *>( raw->dev + ( reinterpret_cast<uint8_t *>( launch_order ) - raw->host ) );

  // ---- device half: arena to HBM on the copy stream, then the header kernels on one of the parse streams ----
  HIP_TRY( hipEventCreateWithFlags( &raw->hdr_done, hipEventDisableTiming ) );
  HIP_TRY( hipMemcpyAsync( raw->dev, raw->host, off, hipMemcpyHostToDevice, ctx->copy ) );
  hipEvent_t up = get_event( ctx );
  HIP_TRY( hipEventRecord( up, ctx->copy ) );
  HIP_TRY( hipStreamWaitEvent( ps, up, 0 ) );
  { bool any_host = false; for ( int i = 0; i < n; i++ ) any_host = any_host || raw->items[i].on_host;
    if ( any_host ) HIP_TRY( hipStreamWaitEvent( ctx->tok.host_up, up, 0 ) ); }      // (the host lanes patch job records the arena's upload carries)
  ctx->free_events.push_back( up );
  const aa::ParseJob * jobs_dev = reinterpret_cast<const aa::ParseJob *>( raw->dev );
  if ( n_order ) {
    LaunchTimer t( ctx, 3, ps );
    if ( int e = aa::launch_parse_mb_headers( jobs_dev, launch_order_dev, n_order, ps ) ) return hip_fail( static_cast<hipError_t>( e ), "k_parse_mb_headers" );
  }
  if ( n_seg_streams ) {
    if ( ctx->last_seg_batch ) HIP_TRY( hipStreamWaitEvent( ps, ctx->last_seg_batch, 0 ) );
    const uint8_t * segs_dev = raw->dev + jobs_bytes + dframes_bytes + sums_bytes;
    if ( int e = aa::launch_segment_fixup( jobs_dev, reinterpret_cast<const aa_seg_stream *>( segs_dev ), n_seg_streams,
                                           reinterpret_cast<const uint32_t *>( segs_dev + size_t( n ) * sizeof( aa_seg_stream ) ), ps ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_segment_fixup" );
    if ( !ctx->last_seg_batch ) HIP_TRY( hipEventCreateWithFlags( &ctx->last_seg_batch, hipEventDisableTiming ) );
    HIP_TRY( hipEventRecord( ctx->last_seg_batch, ps ) );
  }
  raw->ps = ps; raw->launch_order_dev = launch_order_dev; raw->launch_order_host = launch_order; raw->n_order = n_order;
  raw->tokens_pending = true; raw->patch_jobs = defer_tokens;
  HIP_TRY( hipEventRecord( raw->hdr_done, ps ) );  // (the header kernels; recorded again behind the hand-over to the job queue)
  HIP_TRY( hipEventRecord( ctx->parse_idle[pick], ps ) );
  ctx->deferred.push_back( raw );
  abandon.armed = false;                           // the batch is on the books: from here on a failure leaves a consistent state
  // the frames of the host lanes: behind the arena's upload on the copy stream (a worker patches its frame's job record there)
  {
    int n_host = 0;
    for ( int i = 0; i < n; i++ ) if ( raw->items[i].on_host ) n_host++;
    if ( n_host ) {
      host_lanes_start( ctx );
      { std::lock_guard<std::mutex> g( ctx->host_lanes.mu );
        for ( int i = 0; i < n; i++ ) if ( raw->items[i].on_host ) { ctx->host_lanes.backlog_bytes += items[i].size; ctx->host_lanes.q.push_back( { raw, i } ); } }
      ctx->host_lanes.cv.notify_all();
      ctx->stats.host_routed_frames += static_cast<uint64_t>( n_host );
      if ( std::find( ctx->tok.inflight.begin(), ctx->tok.inflight.end(), raw ) == ctx->tok.inflight.end() ) ctx->tok.inflight.push_back( raw );
    }
  }
  if ( !defer_tokens ) if ( aa_status st = launch_tokens_of( ctx, raw ) ) return st;
  if ( first_error != AA_OK ) return fail( first_error, first_message );
  return AA_OK;
}

} // extern "C"
