// runtime.cpp (ABI), between the rasters and the scores: hashes of many rasters / decoders in one call.  The per-stream calls
// (runtime_rasters.inc: slot_hash, state_hash) bring every raster to the host and walk the chain on one core; here every chain that no
// Slot cache answers is a job of ONE k_hash_chains launch (hash_kernels.hip) on a stream of the context's own, the results come back
// through pinned memory, and aa_ctx_hash_wait fills the same Slot caches the per-stream calls read.
namespace {

// The hash stream: the lowest priority the device offers, like the parse streams -- a chain is long and patient
aa_status hash_stream( aa_ctx * ctx )
{
  if ( !ctx->hash.st ) HIP_TRY( hipStreamCreateWithPriority( &ctx->hash.st, hipStreamNonBlocking, ctx->prio_low ) );
  return AA_OK;
}

// what the call needs of the ring: its entry, free (a call that still owns it -- the sixteenth before this one -- is committed first:
// the results are read out of the entry's host memory at the commit, so `done` alone does not free it)
aa_status hash_commit_oldest( aa_ctx * ctx );
aa_status hash_take_buf( aa_ctx * ctx, size_t bytes, int * out )
{
  aa_ctx::Hash & H = ctx->hash;
  while ( static_cast<int>( H.calls.size() ) >= kBindBufs ) if ( aa_status st = hash_commit_oldest( ctx ) ) return st;
  JobRing::Entry * b = nullptr;
  if ( aa_status st = H.ring.take( bytes, size_t( 64 ) << 10, &b, out ) ) return st;
  if ( !H.ready[*out] ) HIP_TRY( hipEventCreateWithFlags( &H.ready[*out], hipEventDisableTiming ) );
  return AA_OK;
}

// The chains of a call under construction: rasters by device pointer (golden is often the raster last is, and every fresh decoder of a
// size points at the context's blank raster: one chain), segment maps one each.
struct HashPlan {
  struct Chain { aa::HashJob job; size_t map_off = 0; bool is_map = false; };
  std::vector<Chain> chains;                      // chain i writes word i of the result table
  std::map<const uint8_t *, int> by_raster;       // device pointer -> chain
  std::map<const uint8_t *, uint64_t> cached;     // ... -> value, for rasters a Slot cache answered
  std::vector<uint8_t> maps;                      // the segment maps, back to back
};

// raster `slot` of s as a value of the call: from its Slot cache, or a chain (new, or the one another raster of the call started)
aa_ctx::Hash::Value hash_plan_raster( aa_ctx * ctx, HashPlan & plan, aa_ctx::Hash::Call & call, aa_stream * s, int slot )
{
  aa_ctx::Hash::Value v;
  const Slot & sl = s->slots[slot];
  retain( s, slot );
  if ( sl.hash_valid ) {
    if ( plan.cached.emplace( sl.dev, sl.hash ).second ) ctx->hash.stats[2]++;
    call.held.push_back( { s, slot, -1 } );
    v.value = sl.hash;
    return v;
  }
  const auto known = plan.cached.find( sl.dev );
  if ( known != plan.cached.end() ) {             // (another decoder's Slot for the same device raster -- the blank one -- had the value)
    Slot & mine = s->slots[slot];
    mine.hash = known->second; mine.hash_valid = true; ctx->hash.stats[3]++;
    call.held.push_back( { s, slot, -1 } );
    v.value = known->second;
    return v;
  }
  auto it = plan.by_raster.find( sl.dev );
  if ( it == plan.by_raster.end() ) {
    HashPlan::Chain c;
    c.job = aa::hash_raster_job( sl.dev, s->plane_bytes[0] + 2 * s->plane_bytes[1], static_cast<uint32_t>( plan.chains.size() ) );
    it = plan.by_raster.emplace( sl.dev, static_cast<int>( plan.chains.size() ) ).first;
    plan.chains.push_back( c );
  }
  call.held.push_back( { s, slot, it->second } );
  v.result = it->second;
  return v;
}

void hash_release_held( aa_ctx::Hash::Call & call )
{
  for ( auto & f : call.held ) release( f.s, f.slot );
  call.held.clear();
}

// Job table, maps and launch of a planned call; the call joins the list of outstanding ones (also when it launches nothing: its
// arrays are written at the wait like every other call's)
aa_status hash_launch( aa_ctx * ctx, HashPlan & plan, aa_ctx::Hash::Call & call )
{
  aa_ctx::Hash & H = ctx->hash;
  const size_t n = plan.chains.size();
  if ( n ) {
    if ( aa_status st = hash_stream( ctx ) ) return st;
    if ( !H.simds ) {
      int cus = 0;
      HIP_TRY( hipDeviceGetAttribute( &cus, hipDeviceAttributeMultiprocessorCount, ctx->device ) );
      H.simds = std::max( 1, cus ) * 4;
      // (ALFALFA_AMD_HASH_SIMDS: as if the chip had that many -- the tests fill waves with lanes of unequal chains at a few dozen jobs)
      if ( const char * e = std::getenv( "ALFALFA_AMD_HASH_SIMDS" ) ) if ( atoi( e ) > 0 ) H.simds = atoi( e );
    }
    const size_t jobs_off = align_up( n * sizeof( uint64_t ) ), maps_off = jobs_off + align_up( n * sizeof( aa::HashJob ) );
    if ( aa_status st = hash_take_buf( ctx, maps_off + plan.maps.size(), &call.buf ) ) return st;
    JobRing::Entry & b = H.ring.entries[call.buf];
    std::memset( b.host, 0, n * sizeof( uint64_t ) );
    if ( !plan.maps.empty() ) std::memcpy( b.host + maps_off, plan.maps.data(), plan.maps.size() );
    // longest chains first: the lanes of a wave get neighbours of the sorted table and finish together
    std::vector<uint32_t> order( n );
    for ( size_t i = 0; i < n; i++ ) order[i] = static_cast<uint32_t>( i );
    std::stable_sort( order.begin(), order.end(), [&]( uint32_t a, uint32_t c ) { return aa::hash_job_steps( plan.chains[a].job ) > aa::hash_job_steps( plan.chains[c].job ); } );
    aa::HashJob * jobs = reinterpret_cast<aa::HashJob *>( b.host + jobs_off );
    uint64_t steps = 0;
    for ( size_t k = 0; k < n; k++ ) {
      const HashPlan::Chain & c = plan.chains[order[k]];
      jobs[k] = c.job;
      if ( c.is_map ) jobs[k].src = b.dev + maps_off + c.map_off;
      steps += aa::hash_job_steps( c.job );
    }
    // every SIMD of the chip has a wave before any wave gets a second lane
    const int lanes_per_wave = static_cast<int>( std::min<size_t>( 64, ( n + H.simds - 1 ) / H.simds ) );
    // behind everything the compute stream holds now: the frames are decoded by then.  Never IN the compute stream: a chain of a
    // 1080p raster runs for tens of milliseconds
    HIP_TRY( hipEventRecord( H.ready[call.buf], ctx->compute ) );
    HIP_TRY( hipStreamWaitEvent( H.st, H.ready[call.buf], 0 ) );
    if ( int e = aa::launch_hash_chains( reinterpret_cast<const aa::HashJob *>( b.dev + jobs_off ), static_cast<int>( n ), lanes_per_wave,
                                         reinterpret_cast<uint64_t *>( b.dev ), H.st ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_hash_chains" );
    call.launched = true;
    if ( aa_status st = H.ring.mark( b, H.st ) ) return st;
    H.stats[0] += n; H.stats[1] += steps;
  } else {
    while ( static_cast<int>( H.calls.size() ) >= kBindBufs ) if ( aa_status st = hash_commit_oldest( ctx ) ) return st;
  }
  H.calls.push_back( std::move( call ) );
  return AA_OK;
}

// The oldest outstanding call: wait for its kernel (the hash stream, not the compute stream), fill the Slot caches, let go of the
// rasters, write the caller's arrays.  The call leaves the list whatever happens, and its rasters are released.
aa_status hash_commit_oldest( aa_ctx * ctx )
{
  aa_ctx::Hash & H = ctx->hash;
  aa_ctx::Hash::Call call = std::move( H.calls.front() );
  H.calls.pop_front();
  struct Held { aa_ctx::Hash::Call & c; ~Held() { hash_release_held( c ); } } held { call };
  const uint64_t * results = nullptr;
  if ( call.launched ) {
    HIP_TRY( hipEventSynchronize( H.ring.entries[call.buf].done ) );
    if ( aa_status st = check_watchdog( ctx ) ) return st;
    results = reinterpret_cast<const uint64_t *>( H.ring.entries[call.buf].host );
  }
  const auto value = [&]( const aa_ctx::Hash::Value & v ) { return v.result >= 0 ? results[v.result] : v.value; };
  for ( auto & f : call.held ) {
    if ( f.result < 0 ) continue;
    Slot & sl = f.s->slots[f.slot];
    if ( !sl.hash_valid ) { sl.hash = results[f.result]; sl.hash_valid = true; H.stats[3]++; }
  }
  if ( call.out ) for ( size_t i = 0; i < call.rasters.size(); i++ ) call.out[i] = value( call.rasters[i] );
  for ( size_t i = 0; i < call.decoders.size(); i++ ) {
    const aa_ctx::Hash::Decoder & d = call.decoders[i];
    uint64_t h[4];
    h[0] = d.state;                                                  // (state_hash: width, height, probability tables so far)
    if ( d.map_result >= 0 ) hcombine( h[0], results[d.map_result] );
    if ( d.filter ) hcombine( h[0], d.filter_hash );
    for ( int k = 0; k < 3; k++ ) h[1 + k] = value( d.refs[k] );
    uint64_t w = 0;
    for ( int k = 0; k < 4; k++ ) hcombine( w, h[k] );
    if ( call.parts ) std::memcpy( call.parts + 4 * i, h, sizeof h );
    if ( call.whole ) call.whole[i] = w;
    if ( call.minihash ) call.minihash[i] = static_cast<uint32_t>( w );
  }
  return AA_OK;
}

void hash_drain( aa_ctx * ctx )
{
  std::lock_guard<std::mutex> g( ctx->hash.mu );
  while ( !ctx->hash.calls.empty() ) (void) hash_commit_oldest( ctx );
}
void hash_free( aa_ctx * ctx )
{
  aa_ctx::Hash & H = ctx->hash;
  if ( H.st ) { (void) hipStreamSynchronize( H.st ); (void) hipStreamDestroy( H.st ); H.st = nullptr; }
  H.ring.destroy();
  for ( hipEvent_t & e : H.ready ) if ( e ) { (void) hipEventDestroy( e ); e = nullptr; }
}

} // namespace

extern "C" {

/* BaseRaster::raw_hash of n decoded frames: out[i] (host) = what aa_stream_raster_hash( streams[i], frame_index[i] ) gives, valid after
 * aa_ctx_hash_wait.  Rasters whose hash is cached launch nothing; the others are one chain each -- one per device raster -- of one
 * kernel on the context's hash stream, behind everything the compute stream holds at the call. */
aa_status aa_hash_rasters_async( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index, uint64_t * out )
{
  if ( !ctx || !streams || !frame_index || !out || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_hash_rasters_async: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  for ( int i = 0; i < n; i++ )
    if ( aa_status st = held_decoded_frame( "aa_hash_rasters_async", ctx, streams[i], frame_index[i], nullptr ) ) return st;
  std::lock_guard<std::mutex> g( ctx->hash.mu );
  HashPlan plan;
  aa_ctx::Hash::Call call;
  call.out = out;
  call.rasters.reserve( n );
  for ( int i = 0; i < n; i++ ) call.rasters.push_back( hash_plan_raster( ctx, plan, call, streams[i], streams[i]->frames[frame_index[i]].out_slot ) );
  const aa_status st = hash_launch( ctx, plan, call );
  if ( st ) hash_release_held( call );
  return st;
}

/* DecoderHash of n decoders (decoder.cc:143-153,482-490): parts[4 i ..] = state, last, golden, alternative; whole[i] = the hash of the
 * four; minihash[i] = its low 32 bits (host arrays, any of them NULL), valid after aa_ctx_hash_wait.  Everything parsed must have
 * been submitted.  The probability tables and the adjustments are hashed on the host here; the segment map of a decoder with
 * segmentation on is a chain of the kernel like the rasters (its current copy travels in the call's pinned buffer). */
aa_status aa_hash_decoders_async( aa_ctx * ctx, aa_stream * const * streams, int n, uint64_t * parts, uint64_t * whole, uint32_t * minihash )
{
  if ( !ctx || !streams || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_hash_decoders_async: bad argument" );
  if ( aa_status st = set_device( ctx ) ) return st;
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = streams[i];
    if ( !s || s->ctx != ctx ) return fail( AA_ERR_ARGUMENT, "aa_hash_decoders_async: stream belongs to another context" );
    if ( s->next_submit != static_cast<int>( s->frames.size() ) ) return fail( AA_ERR_LOGIC, "aa_hash_decoders_async: parsed frames are still waiting to be decoded" );
  }
  for ( int i = 0; i < n; i++ ) if ( aa_status st = segmap_to_host( streams[i] ) ) return st;
  std::lock_guard<std::mutex> g( ctx->hash.mu );
  HashPlan plan;
  aa_ctx::Hash::Call call;
  call.parts = parts; call.whole = whole; call.minihash = minihash;
  call.decoders.resize( n );
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = streams[i];
    const aa::Parser & ps = s->parser;
    aa_ctx::Hash::Decoder & d = call.decoders[i];
    // DecoderState::hash as state_hash (runtime_rasters.inc) forms it; the walk over the segment map is a chain of the kernel
    StateHashParts sp;
    state_hash_parts( ps, sp );
    d.state = sp.head;
    const aa::SegmentationState & sg = ps.segmentation();
    if ( sg.enabled ) {
      HashPlan::Chain c;
      c.is_map = true; c.map_off = plan.maps.size();
      c.job = aa::hash_segment_map_job( nullptr, ps.width(), ps.height(), ps.mb_width(), ps.mb_height(), sp.seg, static_cast<uint32_t>( plan.chains.size() ) );
      const size_t map_bytes = size_t( ps.mb_width() ) * ps.mb_height();
      plan.maps.insert( plan.maps.end(), sg.map.data(), sg.map.data() + map_bytes );
      d.map_result = static_cast<int>( plan.chains.size() );
      plan.chains.push_back( c );
    }
    d.filter = ps.filter_adjustments().enabled; d.filter_hash = sp.filter;
    for ( int k = 0; k < 3; k++ ) d.refs[k] = hash_plan_raster( ctx, plan, call, s, s->cur_ref_slot[k] );
  }
  const aa_status st = hash_launch( ctx, plan, call );
  if ( st ) hash_release_held( call );
  return st;
}

/* Every outstanding hash call: its kernel has run (the hash stream is waited for, not the compute stream), the out arrays are
 * written, the Slot caches filled -- aa_stream_raster_hash / aa_stream_decoder_hash / aa_stream_minihash answer from them without a
 * download -- and the rasters the calls held are let go.  The first error is returned; every call is committed or dropped. */
aa_status aa_ctx_hash_wait( aa_ctx * ctx )
{
  if ( !ctx ) return fail( AA_ERR_ARGUMENT, "null ctx" );
  if ( aa_status st = set_device( ctx ) ) return st;
  std::lock_guard<std::mutex> g( ctx->hash.mu );
  aa_status first = AA_OK;
  std::string message;
  while ( !ctx->hash.calls.empty() ) if ( aa_status st = hash_commit_oldest( ctx ) ) if ( !first ) { first = st; message = g_last_error; }
  return first ? fail( first, message ) : AA_OK;
}

/* out: chains launched, bytes walked (steps of those chains), rasters answered from a Slot cache, Slot cache entries filled */
aa_status aa_ctx_hash_stats( aa_ctx * ctx, uint64_t out[4], int reset )
{
  if ( !ctx || !out ) return fail( AA_ERR_ARGUMENT, "null argument" );
  std::lock_guard<std::mutex> g( ctx->hash.mu );
  std::memcpy( out, ctx->hash.stats, sizeof ctx->hash.stats );
  if ( reset ) std::memset( ctx->hash.stats, 0, sizeof ctx->hash.stats );
  return AA_OK;
}
/* The stream the hash kernels run on (created at the first use; for timing a call with events of the caller's) */
void * aa_ctx_hash_stream( aa_ctx * ctx )
{
  if ( !ctx || set_device( ctx ) ) return nullptr;
  std::lock_guard<std::mutex> g( ctx->hash.mu );
  return hash_stream( ctx ) ? nullptr : ctx->hash.st;
}

} // extern "C"
