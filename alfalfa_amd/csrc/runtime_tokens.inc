// runtime.cpp, one of its pieces: the token workers' host side -- job queue, coefficient heap (virtual range, growth, chunk pool), worker grids
// (launch, top-up, retirement), the mirrored counters, waiting for a frame's `done` word.
namespace {
// ---------------- token workers: job queue, coefficient heap, worker grids ----------------
inline double now_ms() { return std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now().time_since_epoch() ).count(); }
inline aa::Heap heap_of( const aa_ctx * ctx )
{
  aa::Heap h;
  h.base = (AA_GLOBAL int16_t *) ctx->tok.heap; h.pool = (AA_GLOBAL aa::CoeffPool *) ctx->tok.pool; h.ring = (AA_GLOBAL uint32_t *) ctx->tok.ring;
  return h;
}
constexpr size_t kChunkBytesHeap = size_t( aa::kChunkBlocks ) * 32;

// pool_mu held.  Chunk lists of released frames -> one kernel on the COMPUTE stream: behind every reconstruction kernel that
// may still read those coefficients, in front of the event that lets the lists' own memory (the frames' record blocks) go.
void flush_chunk_frees( aa_ctx * ctx )
{
  auto & T = ctx->tok;
  if ( T.pending_lists.empty() ) return;
  if ( aa::launch_pool_free_lists( heap_of( ctx ), T.pending_lists.data(), static_cast<int>( T.pending_lists.size() ), ctx->compute ) == 0 ) T.pending_lists.clear();
  else (void) hipGetLastError();          // (kept: tried again at the next epoch)
}

aa_status tok_refresh_mirror( aa_ctx * ctx )
{
  auto & T = ctx->tok;
  T.mirror_seq++;
  if ( int e = aa::launch_mirror_counters( T.q, T.pool, T.exited_dev, aa_ctx::Tok::kSlots, T.prof_dev, T.mirror_dev, T.mirror_seq, T.util ) )
    return hip_fail( static_cast<hipError_t>( e ), "k_mirror_counters" );
  HIP_TRY( hipStreamSynchronize( T.util ) );
  T.mirror_inflight = false;
  return AA_OK;
}
// ... for callers that only LOOK at the counters (aa_ctx_get_info: a pipelining caller plans by them several times per step): ask
// for a refresh if none is under way, wait for it a few hundred microseconds at most, and otherwise make do with the last one.  On
// an idle GPU the kernel is through in tens of microseconds; beside 700 resident worker workgroups and the reconstruction kernels
// it was seen to take 50-100 ms to get its turn -- 295 ms per step of a caller that waited for it (round 5, profiles/r05_bench_sessions.md).
aa_status tok_peek_mirror( aa_ctx * ctx )
{
  auto & T = ctx->tok;
  if ( !T.mirror_ev ) HIP_TRY( hipEventCreateWithFlags( &T.mirror_ev, hipEventDisableTiming ) );
  if ( !T.mirror_inflight ) {
    T.mirror_seq++;
    if ( int e = aa::launch_mirror_counters( T.q, T.pool, T.exited_dev, aa_ctx::Tok::kSlots, T.prof_dev, T.mirror_dev, T.mirror_seq, T.util ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_mirror_counters" );
    HIP_TRY( hipEventRecord( T.mirror_ev, T.util ) );
    T.mirror_inflight = true;
  }
  const double t0 = now_ms();
  for ( ;; ) {
    const hipError_t e = hipEventQuery( T.mirror_ev );
    if ( e == hipSuccess ) { T.mirror_inflight = false; break; }
    if ( e != hipErrorNotReady ) return hip_fail( e, "hipEventQuery (counters)" );
    (void) hipGetLastError();
    if ( now_ms() - t0 > 0.3 ) break;
    usleep( 20 );
  }
  return AA_OK;
}

// Map more of the heap until `want_mapped` bytes are there (or the memory limit / the reserved range says no).
aa_status tok_grow_heap( aa_ctx * ctx, size_t want_mapped )
{
  auto & T = ctx->tok;
  if ( !T.vmm ) return AA_OK;
  want_mapped = std::min( ( want_mapped + T.grow_bytes - 1 ) / T.grow_bytes * T.grow_bytes, T.heap_va );
  while ( T.heap_mapped < want_mapped ) {
    // (the limit is the pool's too, and the heap never unmaps: a sixteenth of it stays out of the heap's reach, for the arenas and
    // rasters of frames handed over after the heap has taken what it could -- round 4's driver run ended with heap + pool 2.4 GB
    // over a limit the pool could only ask about, not keep)
    { std::lock_guard<std::mutex> g( ctx->pool_mu );
      const size_t reserve = ctx->pool_soft_limit == ~size_t( 0 ) ? 0 : ctx->pool_soft_limit / 16;
      if ( ctx->pool_bytes + T.heap_mapped + T.grow_bytes + reserve > ctx->pool_soft_limit && T.heap_mapped >= T.grow_bytes ) break; }
    hipMemAllocationProp prop {};
    prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = ctx->device;
    hipMemGenericAllocationHandle_t h;
    if ( hipMemCreate( &h, T.grow_bytes, &prop, 0 ) != hipSuccess ) { (void) hipGetLastError(); break; }
    uint8_t * at = T.heap + T.heap_mapped;
    if ( hipMemMap( at, T.grow_bytes, 0, h, 0 ) != hipSuccess ) { (void) hipGetLastError(); (void) hipMemRelease( h ); break; }
    hipMemAccessDesc acc {};
    acc.location.type = hipMemLocationTypeDevice; acc.location.id = ctx->device; acc.flags = hipMemAccessFlagsProtReadWrite;
    if ( hipMemSetAccess( at, T.grow_bytes, &acc, 1 ) != hipSuccess ) { (void) hipGetLastError(); (void) hipMemUnmap( at, T.grow_bytes ); (void) hipMemRelease( h ); break; }
    T.handles.push_back( h );
    if ( int e = aa::launch_pool_push_range( heap_of( ctx ), static_cast<uint32_t>( T.heap_mapped / kChunkBytesHeap ), static_cast<uint32_t>( T.grow_bytes / kChunkBytesHeap ), T.util ) )
      return hip_fail( static_cast<hipError_t>( e ), "k_pool_push_range" );
    T.heap_mapped += T.grow_bytes;
    ctx->stats.heap_grows++;
  }
  return AA_OK;
}

// One tiny kernel per stream of the context, all waiting for each other (k_probe_concurrency): -> how many ran side by side
aa_status probe_stream_concurrency( aa_ctx * ctx )
{
  auto & T = ctx->tok;
  std::vector<hipStream_t> all { ctx->compute, ctx->copy, T.util, T.host_up };
  for ( auto ps : ctx->parse_streams ) all.push_back( ps );
  for ( auto & sl : T.slot ) all.push_back( sl.st );
  const uint32_t n = static_cast<uint32_t>( all.size() );
  uint32_t * d = nullptr;
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( &d ), sizeof( uint32_t ) * ( n + 1 ) ) );
  HIP_TRY( hipMemset( d, 0, sizeof( uint32_t ) * ( n + 1 ) ) );
  HIP_TRY( hipStreamSynchronize( nullptr ) );        // (the memset runs on the null stream and is not ordered against the non-blocking streams the probe runs on)
  for ( uint32_t i = 0; i < n; i++ )
    if ( int e = aa::launch_probe_concurrency( d, d + 1, n, 300000ull /* 3 ms */, static_cast<int>( i ), all[i] ) ) { (void) hipFree( d ); return hip_fail( static_cast<hipError_t>( e ), "k_probe_concurrency" ); }
  for ( auto st : all ) HIP_TRY( hipStreamSynchronize( st ) );
  std::vector<uint32_t> seen( n + 1 );
  HIP_TRY( hipMemcpy( seen.data(), d, sizeof( uint32_t ) * ( n + 1 ), hipMemcpyDeviceToHost ) );
  (void) hipFree( d );
  uint32_t conc = n;
  for ( uint32_t i = 0; i < n; i++ ) conc = std::min( conc, seen[1 + i] );
  ctx->stream_concurrency = conc; ctx->streams_needed = n;
  if ( conc < n ) {
    const std::string msg = "alfalfa_amd: only " + std::to_string( conc ) + " of this context's " + std::to_string( n ) + " HIP streams run side by side (hardware queues): "
                            "set GPU_MAX_HW_QUEUES=16 in the environment before the process initialises HIP (aa_runtime_prepare() does it when called first); "
                            "long-running entropy-decode grids will otherwise hold up reconstruction kernels that share their queue";
    // (said, not refused: in a process with several contexts the streams of all of them share the hardware queues, and a probe
    // kernel that lands behind another context's lingering worker grid also arrives late -- seen in the GPU test session: 7 of 15)
    const char * strict = std::getenv( "ALFALFA_AMD_REQUIRE_QUEUES" );
    if ( strict && atoi( strict ) ) return fail( AA_ERR_LOGIC, msg );
    static std::atomic<bool> said { false };
    if ( !said.exchange( true ) ) std::fprintf( stderr, "%s\n", msg.c_str() );
  }
  return AA_OK;
}

aa_status tok_init( aa_ctx * ctx )
{
  auto & T = ctx->tok;
  if ( T.ready ) return AA_OK;
  hipDeviceProp_t prop;
  HIP_TRY( hipGetDeviceProperties( &prop, ctx->device ) );
  T.n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
  HIP_TRY( hipStreamCreateWithFlags( &T.util, hipStreamNonBlocking ) );
  { int lo = 0, hi = 0; (void) hipDeviceGetStreamPriorityRange( &lo, &hi ); HIP_TRY( hipStreamCreateWithPriority( &T.host_up, hipStreamNonBlocking, hi ) ); }
  for ( auto & sl : T.slot ) HIP_TRY( hipStreamCreateWithPriority( &sl.st, hipStreamNonBlocking, ctx->prio_low ) );
  if ( aa_status st = probe_stream_concurrency( ctx ) ) return st;
  // the job queue
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( &T.q ), 256 ) );
  { aa::TokQueue hq {}; hq.mask = T.q_slots - 1; HIP_TRY( hipMemcpy( T.q, &hq, sizeof hq, hipMemcpyHostToDevice ) ); }
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( &T.slots ), size_t( T.q_slots ) * 8 ) );
  HIP_TRY( hipMemset( T.slots, 0, size_t( T.q_slots ) * 8 ) );
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( &T.one_dev ), 256 ) );
  HIP_TRY( hipMemset( T.one_dev, 0, 256 ) );
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( &T.exited_dev ), sizeof( uint32_t ) * AA_MAX_WORKER_GRIDS ) );
  HIP_TRY( hipMemset( T.exited_dev, 0, sizeof( uint32_t ) * AA_MAX_WORKER_GRIDS ) );
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( &T.cu_slots_dev ), sizeof( uint32_t ) * AA_CU_SLOTS ) );
  HIP_TRY( hipMemset( T.cu_slots_dev, 0, sizeof( uint32_t ) * AA_CU_SLOTS ) );
  if ( const char * e = std::getenv( "ALFALFA_AMD_CU_ADMISSION" ) ) T.cu_cap = std::max( -1, atoi( e ) );
  if ( const char * e = std::getenv( "ALFALFA_AMD_ADMISSION_SURPLUS" ) ) T.cu_surplus = std::max( 0, std::min( 4, atoi( e ) ) );
  if ( const char * e = std::getenv( "ALFALFA_AMD_WORKER_LINGER_MS" ) ) T.linger_ticks = static_cast<unsigned long long>( std::max( 0, atoi( e ) ) ) * 100000ull;
  if ( const char * e = std::getenv( "ALFALFA_AMD_TOPUP_DIV" ) ) T.topup_div = std::max( 1, std::min( 64, atoi( e ) ) );
  if ( const char * e = std::getenv( "ALFALFA_AMD_TOKEN_PROFILE" ) ) if ( atoi( e ) ) {
    HIP_TRY( hipMalloc( reinterpret_cast<void **>( &T.prof_dev ), 64 ) );
    HIP_TRY( hipMemset( T.prof_dev, 0, 64 ) );
  }
  HIP_TRY( hipHostMalloc( reinterpret_cast<void **>( &T.retire_host ), sizeof( uint32_t ) * AA_MAX_WORKER_GRIDS, hipHostMallocDefault ) );
  std::memset( T.retire_host, 0, sizeof( uint32_t ) * AA_MAX_WORKER_GRIDS );
  HIP_TRY( hipHostGetDevicePointer( reinterpret_cast<void **>( &T.retire_dev ), T.retire_host, 0 ) );
  HIP_TRY( hipHostMalloc( reinterpret_cast<void **>( &T.mirror_host ), sizeof( aa_tok_mirror ), hipHostMallocDefault ) );
  std::memset( T.mirror_host, 0, sizeof( aa_tok_mirror ) );
  HIP_TRY( hipHostGetDevicePointer( reinterpret_cast<void **>( &T.mirror_dev ), T.mirror_host, 0 ) );
  // the coefficient heap: a block index is 32 bits and a block 32 bytes -> at most 128 GiB; by default at most 3/4 of what the
  // context may use.  Virtual range now, memory as the frames need it.
  const size_t cap = size_t( 120 ) << 30;
  if ( const char * e = std::getenv( "ALFALFA_AMD_HEAP_GROW_MB" ) ) T.grow_bytes = std::max<size_t>( 2, static_cast<size_t>( atoi( e ) ) ) << 20;     // (tests: small pieces)
  if ( const char * e = std::getenv( "ALFALFA_AMD_HEAP_LIMIT_MB" ) ) T.heap_limit = std::max<size_t>( 2, static_cast<size_t>( atoi( e ) ) ) << 20;
  if ( !T.heap_limit ) T.heap_limit = ctx->pool_soft_limit == ~size_t( 0 ) ? ( size_t( 16 ) << 30 ) : ctx->pool_soft_limit / 4 * 3;
  T.heap_limit = std::max( T.grow_bytes, std::min( cap, T.heap_limit ) / T.grow_bytes * T.grow_bytes );
  const char * no_vmm = std::getenv( "ALFALFA_AMD_NO_VMM" );
  if ( !( no_vmm && atoi( no_vmm ) ) ) {
    void * va = nullptr;
    size_t va_align = 0;
    if ( const char * e = std::getenv( "ALFALFA_AMD_HEAP_VA_ALIGN_MB" ) ) va_align = static_cast<size_t>( atoi( e ) ) << 20;     // (experiments)
    if ( hipMemAddressReserve( &va, T.heap_limit, va_align, nullptr, 0 ) == hipSuccess && va ) { T.heap = static_cast<uint8_t *>( va ); T.heap_va = T.heap_limit; T.vmm = true; }
    else (void) hipGetLastError();
  }
  if ( !T.vmm ) {
    // no virtual memory management on this runtime: one fixed piece (a quarter of the limit unless the caller set one)
    size_t fixed = std::getenv( "ALFALFA_AMD_HEAP_LIMIT_MB" ) ? T.heap_limit : std::max( T.grow_bytes, T.heap_limit / 4 / T.grow_bytes * T.grow_bytes );
    HIP_TRY( hipMalloc( reinterpret_cast<void **>( &T.heap ), fixed ) );
    T.heap_va = fixed;
  }
  // (the token lanes advance a pointer into a chunk with a 32-bit add: tok_fsm.hh bump_words)
  if ( reinterpret_cast<uintptr_t>( T.heap ) & ( kChunkBytesHeap - 1 ) ) return fail( AA_ERR_HIP, "the coefficient heap's base is not aligned to a chunk (64 KB)" );
  uint32_t entries = 1;
  while ( size_t( entries ) * kChunkBytesHeap < T.heap_va ) entries <<= 1;
  uint8_t * pr = nullptr;
  HIP_TRY( hipMalloc( reinterpret_cast<void **>( &pr ), 256 + size_t( entries ) * 4 ) );
  HIP_TRY( hipMemset( pr, 0, 256 + size_t( entries ) * 4 ) );
  T.pool = reinterpret_cast<aa::CoeffPool *>( pr ); T.ring = reinterpret_cast<uint32_t *>( pr + 256 );
  { aa::CoeffPool hp {}; hp.mask = entries - 1; HIP_TRY( hipMemcpy( T.pool, &hp, sizeof hp, hipMemcpyHostToDevice ) ); }
  HIP_TRY( hipStreamSynchronize( nullptr ) );          // (every memset above -- null stream -- has landed before a kernel on a non-blocking stream looks)
  if ( !T.vmm ) {
    if ( int e = aa::launch_pool_push_range( heap_of( ctx ), 0, static_cast<uint32_t>( T.heap_va / kChunkBytesHeap ), T.util ) ) return hip_fail( static_cast<hipError_t>( e ), "k_pool_push_range" );
    T.heap_mapped = T.heap_va;
    { std::lock_guard<std::mutex> g( ctx->pool_mu ); ctx->pool_bytes += T.heap_va; }      // (counts against the memory limit like a slab)
  }
  T.ready = true;
  return AA_OK;
}

void tok_free( aa_ctx * ctx )
{
  auto & T = ctx->tok;
  if ( T.retire_host ) for ( int g = 0; g < aa_ctx::Tok::kSlots; g++ ) __atomic_store_n( &T.retire_host[g], 0xFFFFFFFFu, __ATOMIC_RELEASE );   // lingering workgroups leave now
  if ( T.util ) { (void) hipStreamSynchronize( T.util ); }
  for ( auto & sl : T.slot ) if ( sl.st ) { (void) hipStreamSynchronize( sl.st ); (void) hipStreamDestroy( sl.st ); sl.st = nullptr; }
  if ( T.util ) { (void) hipStreamDestroy( T.util ); T.util = nullptr; }
  if ( T.host_up ) { (void) hipStreamSynchronize( T.host_up ); (void) hipStreamDestroy( T.host_up ); T.host_up = nullptr; }
  if ( T.mirror_ev ) { (void) hipEventDestroy( T.mirror_ev ); T.mirror_ev = nullptr; }
  if ( T.vmm ) {
    if ( T.heap_mapped ) (void) hipMemUnmap( T.heap, T.heap_mapped );
    for ( auto h : T.handles ) (void) hipMemRelease( h );
    if ( T.heap ) (void) hipMemAddressFree( T.heap, T.heap_va );
  } else if ( T.heap ) (void) hipFree( T.heap );
  if ( T.pool ) (void) hipFree( T.pool );
  if ( T.q ) (void) hipFree( T.q );
  if ( T.slots ) (void) hipFree( T.slots );
  if ( T.one_dev ) (void) hipFree( T.one_dev );
  if ( T.exited_dev ) (void) hipFree( T.exited_dev );
  if ( T.cu_slots_dev ) (void) hipFree( T.cu_slots_dev );
  if ( T.prof_dev ) (void) hipFree( T.prof_dev );
  if ( T.retire_host ) (void) hipHostFree( T.retire_host );
  if ( T.mirror_host ) (void) hipHostFree( T.mirror_host );
  const bool packed = T.packed, lpp = T.lane_per_partition;
  T = aa_ctx::Tok {};
  T.packed = packed; T.lane_per_partition = lpp;
}

// Launch worker workgroups if jobs are waiting and fewer workgroups are alive than the GPU holds (the mirror must be fresh).
// `after`: the grid starts behind this event (the hand-over of the jobs it is launched for).
aa_status tok_launch_workers( aa_ctx * ctx, hipEvent_t after )
{
  auto & T = ctx->tok;
  const aa_tok_mirror & M = *T.mirror_host;
  const int32_t queued = static_cast<int32_t>( static_cast<uint32_t>( T.jobs_enqueued ) - M.q_head );
  if ( queued <= 0 || T.lanes < 1 ) return AA_OK;
  int alive[aa_ctx::Tok::kSlots], alive_total = 0;
  for ( int g = 0; g < aa_ctx::Tok::kSlots; g++ ) {
    alive[g] = static_cast<int>( T.slot[g].launched - M.exited[g] );
    if ( T.slot[g].queued_behind_retiring && static_cast<int32_t>( M.exited[g] - T.slot[g].retiring_until ) >= 0 ) T.slot[g].queued_behind_retiring = false;
    alive_total += alive[g];
  }
  // as many workgroups as there are jobs waiting, up to what the GPU holds: when lanes are plentiful a frame gets a wave of its
  // own (a wave steps faster the fewer lanes it carries); grids already launched for these jobs -- started or not -- count
  // (round 6: a BIG hand-over gets the whole GPU's worth of workgroups in ONE grid.  With the exact LDS request four worker workgroups fit
  // a CU where the shape wants three, and what keeps it at three is that the dispatcher spreads the workgroups of one grid evenly;
  // several grids launched one after the other as the first hand-overs of a run arrive -- 480 key frames, then 5 280 inter frames --
  // pile up unevenly, and the row kernels' hand-off chains run at the pace of the CUs with the least LDS left: the runs that started
  // with many grids were the slow ones, profiles/r06_bench_sessions.md sessions 8-10)
  const bool whole_gpu = queued * 2 >= T.cap_wgs;
  int want = ( whole_gpu ? T.cap_wgs : std::min( T.cap_wgs, queued ) ) - alive_total;
  // ... and not in dribs and drabs: a grid takes a worker stream for as long as its last wave lives, so small top-ups use the
  // streams up.  Waves linger when the queue is empty; a top-up is for when a good part of the GPU's lanes is really gone.
  if ( want <= 0 || ( alive_total > 0 && want * T.topup_div < T.cap_wgs && want < queued ) ) return AA_OK;
  int g = -1;
  for ( int k = 0; k < aa_ctx::Tok::kSlots; k++ ) if ( alive[k] == 0 ) { g = k; break; }
  if ( g < 0 ) {
    // every worker stream still has a grid with workgroups alive (remnants that keep taking jobs would hold their stream for
    // good): the smallest one retires -- its lanes finish the frames they have and take no more -- and the new grid queues behind it
    for ( int k = 0; k < aa_ctx::Tok::kSlots; k++ )
      if ( !T.slot[k].queued_behind_retiring && ( g < 0 || alive[k] < alive[g] ) ) g = k;
    // (a retiring grid's lanes stop taking frames and the new grid starts when the old one's last chain has ended: that costs capacity
    // for up to a key frame's chain -- worth it when half the GPU's lanes are gone, or when the grid that goes is small beside what
    // comes.  Without the second case a long run whose waves leave after a short linger would end up with every worker stream held
    // by a remnant and no way to top up before half the lanes are gone.)
    if ( g < 0 ) return AA_OK;
    const bool half_gone = alive[g] * 4 <= T.cap_wgs && alive_total * 2 <= T.cap_wgs;
    const bool small_remnant = alive[g] * 2 <= want;
    if ( !half_gone && !small_remnant ) return AA_OK;
    __atomic_store_n( &T.retire_host[g], T.slot[g].gen, __ATOMIC_RELEASE );
    T.slot[g].queued_behind_retiring = true; T.slot[g].retiring_until = T.slot[g].launched;
    ctx->stats.worker_retires++;
    want = std::min( T.cap_wgs, want + alive[g] );       // (the remnant's workgroups are gone by the time this grid starts)
  }
  auto & sl = T.slot[g];
  sl.gen++;
  // Per-CU admission (k_token_workers): the shape wants per_cu workgroups on a CU; when the LDS request would let one more in, a workgroup
  // that lands on a CU that has its share leaves at once and is replaced by a top-up.  Measured (profiles/r06_bench_sessions.md, session
  // 11): 145.3 / 144.4 / 144.3 M macroblocks/s with the admission, 127.7 / 134.3 / 141.0 / 141.7 / 129.3 M without -- the slow runs are the
  // ones in which overlapping grids left some CUs with four worker workgroups and the row kernels' hand-off chains ran at those CUs' pace.
  const int per_cu = T.n_cus > 0 ? T.cap_wgs / T.n_cus : 0;
  const uint32_t cu_cap = T.cu_cap >= 0 ? static_cast<uint32_t>( T.cu_cap )
                                        : ( per_cu > 0 && static_cast<size_t>( T.lds ) * static_cast<size_t>( per_cu + 1 ) <= size_t( 160 ) * 1024 ? static_cast<uint32_t>( per_cu ) : 0u );
  // (ALFALFA_AMD_ADMISSION_SURPLUS=n, experiments: the grid launched with n more workgroups per CU than wanted, so that every CU is offered
  // one more than it may keep -- the dispatcher does not place a grid evenly when other kernels hold resources at that moment.  Measured,
  // sessions 13-16: the first step starts with all 768 workgroups, but the steady count is set by the top-up threshold either way
  // (680-690 alive) and the end-to-end figure is the same within the run-to-run spread: off by default.  And the only two runs of the
  // round that were lost to an expired row-kernel wait both had it on (DESIGN.md 4.1, "A second look"): do not turn it on in production.)
  if ( cu_cap && whole_gpu ) want += T.n_cus * T.cu_surplus;      // (small calls: a workgroup per frame, nothing to even out)
  if ( after ) HIP_TRY( hipStreamWaitEvent( sl.st, after, 0 ) );
  LaunchTimer timer( ctx, 4, sl.st );
  if ( int e = aa::launch_token_workers( T.q, T.slots, heap_of( ctx ), T.exited_dev + g, T.retire_dev + g, sl.gen, static_cast<uint32_t>( T.cap_wgs ), T.prof_dev, T.linger_ticks, want, T.lanes, T.lane_bytes, T.lds, T.packed, T.lane_per_partition ? T.mp_hint : 0u, sl.st, T.cu_slots_dev, cu_cap ) )
    return hip_fail( static_cast<hipError_t>( e ), "k_token_workers" );
  sl.launched += static_cast<uint32_t>( want );
  ctx->stats.worker_launches++; ctx->stats.worker_wgs += static_cast<uint64_t>( want );
  return AA_OK;
}

// What a waiting host does every few milliseconds: look at the device's counters, map more heap when lanes starve, make sure
// workgroups exist for the jobs that wait.
aa_status tok_service( aa_ctx * ctx, hipEvent_t after = nullptr )
{
  auto & T = ctx->tok;
  if ( !T.ready ) return AA_OK;
  if ( aa_status st = tok_peek_mirror( ctx ) ) return st;       // (a look, not a wait: this runs inside every wait for a frame's parse)
  if ( T.mirror_host->pool_starving != T.seen_starving ) {
    T.seen_starving = T.mirror_host->pool_starving;
    if ( aa_status st = tok_grow_heap( ctx, T.heap_mapped + T.grow_bytes ) ) return st;
  }
  return tok_launch_workers( ctx, after );
}

inline double parse_timeout_ms()
{
  static const double ms = [] { const char * e = std::getenv( "ALFALFA_AMD_PARSE_TIMEOUT_S" ); const double s = e ? atof( e ) : 0.0; return ( s > 0 ? s : 300.0 ) * 1000.0; }();
  return ms;
}
// the token lane's `done` word of one frame (pinned host memory the lane writes last)
// (the `done` word is the writer's last store behind a release -- a GPU lane's system-scope fence, a host lane's thread fence: read
// it with acquire, so that what the reader looks at next -- the summary's counts, host_dense -- is what the writer left)
inline bool summary_done( volatile aa::FrameSummary * sum ) { return __atomic_load_n( const_cast<const uint32_t *>( &sum->done ), __ATOMIC_ACQUIRE ) != 0; }
aa_status tok_wait_done( aa_ctx * ctx, volatile aa::FrameSummary * sum )
{
  if ( summary_done( sum ) ) return AA_OK;
  const double t0 = now_ms();
  double last = t0 - 1e9;
  int spins = 0;
  while ( !summary_done( sum ) ) {
    const double t = now_ms();
    if ( t - last > 2.0 ) { if ( aa_status st = tok_service( ctx ) ) return st; last = t; }
    if ( t - t0 > parse_timeout_ms() ) return fail( AA_ERR_HIP, "device parser: a frame handed to the token workers was not finished in time (ALFALFA_AMD_PARSE_TIMEOUT_S, default 300)" );
    if ( ++spins > 64 ) usleep( 50 );
  }
  ctx->stats.parse_wait_ms += now_ms() - t0;
  return AA_OK;
}

// every frame handed to the queue so far is through
bool batch_through( const Batch * b )
{
  const volatile aa::FrameSummary * sums = reinterpret_cast<const volatile aa::FrameSummary *>( b->host + b->summaries_off );
  for ( int i = 0; i < b->n; i++ ) if ( b->items[i].live && b->items[i].s->frames[b->items[i].frame].enqueued && !sums[i].done ) return false;
  return true;
}
aa_status tok_quiesce( aa_ctx * ctx )
{
  auto & T = ctx->tok;
  for ( Batch * b : T.inflight ) {
    volatile aa::FrameSummary * sums = reinterpret_cast<volatile aa::FrameSummary *>( b->host + b->summaries_off );
    for ( int i = 0; i < b->n; i++ )
      if ( b->items[i].live && b->items[i].s->frames[b->items[i].frame].enqueued ) if ( aa_status st = tok_wait_done( ctx, &sums[i] ) ) return st;
  }
  T.inflight.clear();
  return AA_OK;
}
void tok_prune_inflight( aa_ctx * ctx )
{
  auto & v = ctx->tok.inflight;
  if ( v.size() < 64 ) return;
  size_t keep = 0;
  for ( Batch * b : v ) if ( !batch_through( b ) ) v[keep++] = b;
  v.resize( keep );
}

// The slice of LDS a token lane needs depends on the widest frame (its above-row flags) and on whether frames have several DCT
// partitions.  Grids with smaller slices cannot run such frames, so the size only ever grows -- and before it does, the queue
// is drained and the grids are gone.
aa_status tok_set_lane_bytes( aa_ctx * ctx, uint32_t need )
{
  auto & T = ctx->tok;
  if ( need <= T.lane_bytes ) return AA_OK;
  if ( T.lane_bytes ) {
    if ( aa_status st = tok_quiesce( ctx ) ) return st;
    // the grids that linger (idle waves stay for `linger`) are told to leave now: nobody should wait that long for them
    for ( int g = 0; g < aa_ctx::Tok::kSlots; g++ ) {
      auto & sl = T.slot[g];
      __atomic_store_n( &T.retire_host[g], sl.gen, __ATOMIC_RELEASE );
      sl.gen++;                                         // (the next grid of this slot is of a generation the word does not cover)
    }
    for ( auto & sl : T.slot ) HIP_TRY( hipStreamSynchronize( sl.st ) );
    for ( auto & sl : T.slot ) { sl.queued_behind_retiring = false; }
  }
  T.lane_bytes = ( need + 15u ) & ~15u;
  int per_cu = 0;
  aa::token_worker_shape( T.lane_bytes, T.n_cus, &T.lanes, &T.lds, &per_cu );
  if ( T.lanes < 1 || per_cu < 1 ) return fail( AA_ERR_UNSUPPORTED, "device parser: a token lane for frames this wide does not fit a workgroup's LDS" );
  T.cap_wgs = per_cu * T.n_cus;
  return AA_OK;
}

} // namespace
