// runtime.cpp, the first of its pieces (one translation unit, #included in order by runtime.cpp): error reporting, the cores a process
// really gets, and the records behind the ABI -- the ring of pinned job tables, frame-store chunks, the batch of a submit call, raster
// slots, frame records, the context (aa_ctx: streams, device pool, token-worker state, host lanes) and the stream (aa_stream).
namespace {

thread_local std::string g_last_error;

// The entropy-decode kernels are long (a chain per lane, seconds) and must run BESIDE reconstruction and beside each other.
// HIP spreads streams over few hardware queues by default (4), and commands of one queue run in order: with more streams
// than queues a decode launch can end up queued behind a parse kernel.  The number of queues is read from the environment
// (GPU_MAX_HW_QUEUES) when the HIP runtime starts.  The library does not touch the host process's environment behind its back:
// aa_runtime_prepare() -- called by the bindings before their first aa_ctx_create, or by the host program before ITS first HIP
// call -- sets the variable if it is unset; a context then CHECKS how many of its streams really run side by side
// (probe_stream_concurrency) and says so: aa_ctx_info::stream_concurrency, a warning on stderr below 8 -- an error only with
// ALFALFA_AMD_REQUIRE_QUEUES=1 (several contexts of one process share the queues and a probe can arrive late behind another's grid).

aa_status fail( aa_status code, const std::string & msg ) { g_last_error = msg; return code; }

// Cores this process can really use: what the OS shows (hardware_concurrency, the affinity mask) bounded by the cgroup CPU quota.
// Round 4's GPU box shows 256 hardware threads under a quota of 16 CPUs (cpu.max = "1600000 100000"): 256 parser threads there get
// through LESS than 32 do (tools/host_parallelism.py: 25x one thread at 16-64 threads, 22x at 256), and a plan that counts on 256
// cores is off by 16x.
int effective_cpus()
{
  static const int n = [] {
    int cpus = static_cast<int>( std::thread::hardware_concurrency() );
    if ( cpus < 1 ) cpus = 1;
    cpu_set_t set;
    if ( sched_getaffinity( 0, sizeof set, &set ) == 0 ) { const int a = CPU_COUNT( &set ); if ( a > 0 && a < cpus ) cpus = a; }
    auto read_two = []( const char * path, double * a, double * b ) -> int {
      FILE * f = std::fopen( path, "r" );
      if ( !f ) return 0;
      char first[64] = { 0 };
      int got = std::fscanf( f, "%63s %lf", first, b );
      std::fclose( f );
      if ( got < 1 ) return 0;
      if ( std::strcmp( first, "max" ) == 0 ) { *a = -1; return got; }
      *a = atof( first );
      return got;
    };
    double quota = -1, period = 100000;
    if ( read_two( "/sys/fs/cgroup/cpu.max", &quota, &period ) < 1 ) {                 // cgroup v2; else v1
      double q = -1, dummy = 0;
      if ( read_two( "/sys/fs/cgroup/cpu/cpu.cfs_quota_us", &q, &dummy ) >= 1 ) { quota = q; double pp = 100000; if ( read_two( "/sys/fs/cgroup/cpu/cpu.cfs_period_us", &pp, &dummy ) >= 1 && pp > 0 ) period = pp; }
    }
    if ( quota > 0 && period > 0 ) { const int q = std::max( 1, static_cast<int>( quota / period + 0.5 ) ); if ( q < cpus ) cpus = q; }
    return cpus;
  }();
  return n;
}
// host workers of one call: what the caller asked for (0: all), never more than twice the cores the process really gets
int worker_threads( int asked )
{
  const int cap = std::max( 1, std::min( 256, 2 * effective_cpus() ) );
  return std::max( 1, std::min( asked > 0 ? asked : cap, cap ) );
}
aa_status hip_fail( hipError_t e, const char * what )
{
  return fail( e == hipErrorNoDevice || e == hipErrorInvalidDevice ? AA_ERR_NO_DEVICE : AA_ERR_HIP,
               std::string( what ) + ": " + hipGetErrorString( e ) );
}
#define HIP_TRY( expr ) do { hipError_t e__ = ( expr ); if ( e__ != hipSuccess ) return hip_fail( e__, #expr ); } while ( 0 )

constexpr size_t kChunkBytes = size_t( 64 ) << 20;
constexpr size_t kAlign = 256;
inline size_t align_up( size_t v, size_t a = kAlign ) { return ( v + a - 1 ) / a * a; }

// boost::hash_combine / hash_range as the reference uses them (pre-1.81 formula)
inline void hcombine( uint64_t & seed, uint64_t v ) { seed ^= v + 0x9e3779b9ull + ( seed << 6 ) + ( seed >> 2 ); }
inline void hrange_u8( uint64_t & seed, const uint8_t * p, size_t n ) { for ( size_t i = 0; i < n; i++ ) hcombine( seed, p[i] ); }
inline void hrange_i8( uint64_t & seed, const int8_t * p, size_t n ) { for ( size_t i = 0; i < n; i++ ) hcombine( seed, static_cast<uint64_t>( static_cast<int64_t>( p[i] ) ) ); }

// The job table of a batched call (raster bindings, gather list, render jobs, scoring jobs, hash chains) is written by the host and
// read by the device, and the host runs ahead of the device: each kind of call has a ring of kBindBufs pinned tables.  `done` is
// recorded (mark) behind the last device command that reads the table; take() waits for it when the entry comes round again.
constexpr int kBindBufs = 16;               // calls of one kind the host may run ahead of the device
struct JobRing {
  struct Entry {
    uint8_t * host = nullptr;               // pinned
    uint8_t * dev = nullptr;                // `host` as the device sees it: what a kernel that reads the table over the bus is given
    size_t cap = 0;                         // bytes
    hipEvent_t done = nullptr;
    bool busy = false;
  };
  Entry entries[kBindBufs];
  int next = 0;                             // the entry the next take() hands out
  // The next entry, free and with room for `bytes` (grown to twice the need, at least floor_bytes); *waited_ms: the wait for its last user
  aa_status take( size_t bytes, size_t floor_bytes, Entry ** out, int * index = nullptr, double * waited_ms = nullptr )
  {
    const int i = next;
    Entry & e = entries[i];
    next = ( next + 1 ) % kBindBufs;
    if ( e.busy ) {
      const auto t0 = std::chrono::steady_clock::now();
      HIP_TRY( hipEventSynchronize( e.done ) );
      e.busy = false;
      if ( waited_ms ) *waited_ms = std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now() - t0 ).count();
    }
    if ( e.cap < bytes ) {
      if ( e.host ) (void) hipHostFree( e.host );
      e.host = e.dev = nullptr; e.cap = 0;
      const size_t cap = align_up( std::max( floor_bytes, bytes * 2 ) );
      HIP_TRY( hipHostMalloc( reinterpret_cast<void **>( &e.host ), cap, hipHostMallocDefault ) );
      HIP_TRY( hipHostGetDevicePointer( reinterpret_cast<void **>( &e.dev ), e.host, 0 ) );
      e.cap = cap;
    }
    if ( !e.done ) HIP_TRY( hipEventCreateWithFlags( &e.done, hipEventDisableTiming ) );
    *out = &e;
    if ( index ) *index = i;
    return AA_OK;
  }
  // `st` has been given the last command that reads the entry's table
  aa_status mark( Entry & e, hipStream_t st ) { HIP_TRY( hipEventRecord( e.done, st ) ); e.busy = true; return AA_OK; }
  void destroy()
  {
    for ( Entry & e : entries ) { if ( e.host ) (void) hipHostFree( e.host ); if ( e.done ) (void) hipEventDestroy( e.done ); e = Entry(); }
  }
};

struct Chunk {
  uint8_t * host = nullptr;   // pinned
  uint8_t * dev = nullptr;
  size_t capacity = 0, used = 0, uploaded = 0;
  size_t pinned_bytes = 0;    // size of the host allocation (capacity shrinks to `used` when the chunk is sealed)
  size_t dev_bytes = 0;       // size of the device piece
  int live_frames = 0;        // frames whose records live here and have not been released
};

// One aa_submit_frames call: a pinned arena mirrored in HBM holding the parse jobs, the reconstruction job records, the
// result summaries and the compressed frames themselves; the device parser writes each frame's records into that frame's own
// record block.  Lives until the last of its frames is released.
struct Batch {
  uint8_t * host = nullptr, * dev = nullptr;
  size_t host_bytes = 0, dev_bytes = 0;
  int n = 0, live = 0;
  hipEvent_t hdr_done = nullptr;             // macroblock-header kernel (+ segment pass, + the hand-over to the job queue) finished
  size_t summaries_off = 0;
  uint8_t * host_dev = nullptr;              // `host` as the device sees it (the parse kernels write the summaries there)
  // Two-phase form (AA_SUBMIT_DEFER_TOKENS): the macroblock-header kernel has been queued, the token kernel has not -- the
  // coefficient blocks (9/10 of a frame's records) are only allocated when it is (aa_launch_tokens, or the first call that
  // needs the frame's records).
  bool tokens_pending = false;
  bool patch_jobs = false;                   // the jobs in HBM lack the coefficient pointers (two-phase form)
  size_t head_bytes = 0;                     // parse jobs + reconstruction job records at the start of the arena
  const uint32_t * launch_order_dev = nullptr;
  uint32_t * launch_order_host = nullptr;    // ... in the pinned half: the LIVE items only, longest chains first
  int n_order = 0;                           // entries of the launch order (frames the pre-pass rejected are not in it)
  int max_mbw = 0, max_nparts = 1;
  hipStream_t ps = nullptr;
  int parse_stream_index = 0;
  // on_host: the frame was handed to a HOST LANE, not to the GPU's job queue (host_lane_run): its dense coefficient blocks are a
  // pool piece of its own (host_dense: written by the worker before the frame's `done` word, read after it)
  struct Item { aa_stream * s; int frame; bool live; bool on_host = false; size_t data_off = 0; uint8_t * host_dense = nullptr; size_t host_dense_bytes = 0; };
  std::vector<Item> items;                   // [n]; live: accepted and not released since
};

// A raster: three padded planes in one piece of the context's device pool.  The piece goes back to the pool when the last
// holder lets go (RasterHandle semantics, raster_handle.cc:113-122) -- rasters are pooled per GPU, not per stream, so a stream
// that is idle between two groups of pictures holds one raster (its last reference), not a private stock.
struct Slot {
  uint8_t * dev = nullptr;    // null: a free entry of the stream's slot table
  bool shared = false;        // the context's blank raster of this size (what a new decoder's references point at): not this stream's to free
  int refs = 0;               // References + frame handles holding this raster
  bool hash_valid = false;    // HashCachedRaster: the hash is computed once per raster (raster_handle.cc:196-206)
  uint64_t hash = 0;
};

struct FrameRec {
  aa_frame_header hdr;
  aa_dev_frame * host_job = nullptr;       // in pinned chunk
  const aa_dev_frame * dev_job = nullptr;  // same offset in device chunk
  int out_slot = -1;
  int ref_after[3] = { -1, -1, -1 };       // References (last, golden, alt) after this frame, as frame indices
  std::vector<uint8_t> intra_diagonals;    // [d] != 0: diagonal d holds an intra MB
  bool has_split = false;                  // some macroblock is SPLITMV (handled by the one-macroblock-per-wave kernel)
  bool handle_held = true;
  int chunk = -1;                          // host-parsed frame: index of the frame-store chunk holding its records
  Batch * batch = nullptr;                 // device-parsed frame: its submit call ...
  int batch_item = -1;                     // ... and its index there
  bool summary_pending = false;            // counts (intra macroblocks, coefficient blocks, SPLITMV) not yet read back from the device parser
  uint8_t * rec_block = nullptr;           // device-parsed frame: macroblock records, intra row masks, flags, chunk list in HBM
  size_t rec_bytes = 0;
  bool rec_in_arena = false;               // ... inside the device half of its batch's arena (freed with the batch)
  const uint32_t * chunk_list = nullptr;   // ... the list of coefficient chunks its token lane took (in rec_block; [0] = count)
  aa_mb_info * dev_mbs = nullptr;          // ... its macroblock records (in rec_block)
  const uint32_t * packed_pos = nullptr;   // ... packed coefficient storage: where every macroblock's words start (in rec_block); null: dense blocks
  volatile aa::FrameSummary * summary = nullptr;   // in the batch's pinned arena: the token lane's last word lands here
  const aa::ParseJob * parse_job = nullptr;        // in the batch's device arena
  bool enqueued = false;                   // handed to the job queue (a token lane may be writing its records)
  uint32_t est_chunks = 0;                 // coefficient chunks accounted for this frame (an estimate until the parse is over)
  bool chunks_returned = false;            // the frame was handed back for lack of memory and its chunks are in the pool again
  bool records_released = false;
  bool placed = false;                     // raster slot + References bookkeeping done (at the first decode submission)
};

} // namespace

struct aa_parser { aa::Parser impl; aa_parser( uint16_t w, uint16_t h ) : impl( w, h ) {} };

struct aa_ctx {
  int device = 0;
  hipStream_t compute = nullptr, copy = nullptr;
  hipEvent_t upload_done = nullptr;
  std::atomic<int> refs { 1 };   // the context handle + one per stream: freed by whoever drops the last (bindings may finalise in any order)
  // device-side entropy decode: submit calls rotate over a few HIP streams so that the parse of one batch runs beside the
  // parse of the next and beside reconstruction (a parse is a few thousand latency-bound chains, not a chip-filling kernel)
  JobRing bind_ring;                        // the raster bindings of an aa_decode_batch call (bind_batch), read by k_bind_rasters over the bus
  // HOST LANES: host cores in the role of token lanes.  A frame handed to them (AA_SUBMIT_HOST on a call with many streams: the key
  // frames a pipeline needs at once -- 35 ms on a core, 2 s as a chain on a GPU lane) has had its header pre-pass like every frame
  // of the device route; a worker thread parses macroblock headers and tokens from the batch arena's pinned copy (aa::parse_frame_body),
  // uploads the records to where the kernels expect them and then writes the SAME `done` word a GPU lane writes -- the submit call does
  // not wait, and everything that waits for a frame's parse (aa_decode_batch, aa_stream_frame_header, release) waits for that word.
  struct HostLanes {
    struct Task { Batch * b; int item; };
    std::mutex mu; std::condition_variable cv;
    std::deque<Task> q;
    std::vector<std::thread> threads;
    bool stop = false;
    // what the workers have really achieved (parse time only: no allocation, no upload) and what they have been given and not finished
    std::atomic<uint64_t> parsed_bytes { 0 }, parse_us { 0 }, backlog_bytes { 0 };
    uint64_t parse_us_mark = 0;          // parse_us at the last aa_ctx_kernel_stats reset
  } host_lanes;
  // the raster list of a batched download (aa_download_batch_async), read by k_gather_rasters over the bus; gather_copied[i]: recorded
  // on the COPY stream behind the copy of the call that has entry i (downloads_in_flight lists such entries)
  JobRing gather_ring;
  hipEvent_t gather_copied[kBindBufs] = {};
  // the float table and job list of a render (aa_render_rgb_async) and the job table of a scoring call (quality_of_planes): copied on
  // the compute stream into the call's piece of the device pool; `done` fires when the copy has read the entry
  JobRing rgb_ring, quality_ring;
  double rebase_timing[5] = {};             // aa_rebase_last_timing
  double reencode_timing[5] = {};           // aa_reencode_last_timing
  double encode_timing[5] = {};             // aa_encode_last_timing
  double serialize_timing[5] = {};          // aa_serialize_last_timing
  int reenc_slots = 16;                     // macroblocks of an anti-diagonal per round of k_reencode_inter, k_encode_key and k_encode_inter (aa_ctx_set_reencode_slots)
  int lf_round = 4;                         // aa_lf_search_decode_batch: levels per job and round; lf_jobs_per_slice: jobs per slice, 0 = by memory (aa_ctx_set_lf_search_round)
  int lf_jobs_per_slice = 0;
  double lf_timing[8] = {};                 // aa_lf_search_last_timing
  int target_jobs_per_slice = 0;            // aa_estimate_size_batch / aa_target_size_batch: jobs per slice of a round, 0 = by memory (aa_ctx_set_target_size_round)
  double target_size_timing[6] = {};        // aa_target_size_last_timing
  JobRing lf_ring;                          // a slice's job table, states and round tables of aa_lf_search_decode_batch, copied on the compute stream into the slice's piece
  JobRing rebase_ring;                     // the job table and input records of a rebase slice (aa_rebase_batch), copied on the compute stream into the slice's piece
  hipEvent_t rgb_consumer_ev = nullptr, quality_consumer_ev = nullptr;   // stream_waits_for: the caller's stream and the compute stream waiting for each other
  // batched hashes (runtime_hashes.inc): a stream of their own, a ring of pinned tables (result table, job table, segment maps: read
  // and written by k_hash_chains over the bus; an entry is its call's until hash_commit_oldest has read the results out of it) and the
  // calls whose results nobody has committed yet, oldest first.  ready[i]: compute stream -> hash stream, for the call that has entry i
  struct Hash {
    struct Value { uint64_t value = 0; int result = -1; };      // result >= 0: word `result` of the call's result table, else `value`
    struct Fill { aa_stream * s; int slot; int result; };        // a raster the call holds; result >= 0: its Slot cache is filled at the wait
    struct Decoder { uint64_t state = 0; int map_result = -1; bool filter = false; uint64_t filter_hash = 0; Value refs[3]; };
    struct Call {
      int buf = -1; bool launched = false;
      std::vector<Fill> held;
      std::vector<Value> rasters; uint64_t * out = nullptr;                                   // aa_hash_rasters_async
      std::vector<Decoder> decoders; uint64_t * parts = nullptr, * whole = nullptr; uint32_t * minihash = nullptr;   // aa_hash_decoders_async
    };
    std::mutex mu;
    hipStream_t st = nullptr;
    JobRing ring;
    hipEvent_t ready[kBindBufs] = {};
    int simds = 0;
    std::deque<Call> calls;
    uint64_t stats[4] = { 0, 0, 0, 0 };      // chains launched, bytes walked, rasters answered from the cache, cache entries filled
  } hash;
  int row_handoff_by_kernel[2] = { 0, 0 };   // (diagnostics: waits the second look ended, k_recon_intra4 / k_loopfilter_rows4)
  std::deque<int> downloads_in_flight;   // gather_ring entries whose copy (aa_download_batch_async) nobody has waited for yet, oldest first
  // A parse batch holds its stream for as long as its longest chain (seconds for a key frame): a batch queued behind another
  // one on the same stream starts that much later.  Hence one stream per batch that can be in flight, and a batch goes to a
  // stream that has nothing queued (pick_parse_stream).
  static constexpr int kMaxParseStreams = 20;
  // Hardware queues are few (16 asked for above) and a queue runs its commands in order: a stream that shares a queue with a
  // worker grid -- which stays for as long as there is work -- would not get a kernel started until that grid leaves.  So the
  // context keeps to 16 streams: compute, copy, utility, expansion, 4 header-parse streams (short kernels now), 8 worker streams.
  int n_parse_streams = 4;
  std::vector<hipStream_t> parse_streams;
  std::vector<hipEvent_t> parse_idle;    // recorded behind the last operation queued on the stream
  int prio_low = 0;
  int next_parse_stream = 0;
  hipEvent_t last_seg_batch = nullptr;  // segment-map passes of consecutive batches must run in order
  std::vector<Batch *> deferred;        // batches whose frames have not been handed to the job queue yet, oldest first
  // ---- token workers: job queue, coefficient heap, worker grids (tok_fsm.hh) ----
  struct Tok {
    bool ready = false;
    hipStream_t util = nullptr;          // mirror kernel, heap pushes: never behind anything long
    hipStream_t host_up = nullptr;       // the HOST LANES' uploads (records, dense blocks, the job-record patch of a frame a host core parsed): a stream of their
                                         // own since round 6 (the hardware queue the expansion kernels of rounds 4-5 had).  On the copy stream -- which is also the
                                         // download stream, whose copies wait for compute-stream events -- a key frame's `done` word waited behind every queued
                                         // raster download and the reconstruction backlog in front of it (ADVICE round 5)
    // job queue
    aa::TokQueue * q = nullptr;
    unsigned long long * slots = nullptr;
    uint32_t q_slots = 1u << 18;
    uint64_t jobs_enqueued = 0;          // tickets the host has scheduled (a ticket = one frame, rejected ones included)
    std::vector<Batch *> inflight;       // batches with frames handed to the queue that may not be through yet (a batch leaves when it dies)
    std::vector<Batch *> batches;        // every live batch whose frames went to the queue, oldest first (eviction walks it from the back)
    uint32_t * one_dev = nullptr;        // a zero in HBM: the `order` of a one-job hand-over
    // coefficient heap: ONE virtual range, physical memory mapped as the frames need it
    uint8_t * heap = nullptr;
    size_t heap_va = 0, heap_mapped = 0, heap_limit = 0, grow_bytes = size_t( 1 ) << 30;
    bool vmm = false;
    std::vector<hipMemGenericAllocationHandle_t> handles;
    aa::CoeffPool * pool = nullptr;
    uint32_t * ring = nullptr;
    int64_t chunks_committed = 0;        // chunks frames hold (parsed: what they took) or are expected to take (in flight: estimate)
    double blocks_per_byte = 1.0;        // running estimate: coefficient blocks a frame stores per byte of its compressed size (never more than 25 per macroblock)
    // Packed coefficient storage (tok_fsm.hh): the lanes write a mask word + the non-zero coefficients of a block instead of 16
    // coefficients; frames are expanded into a transient dense array when they are handed to reconstruction.  One format per
    // context, fixed when the first frame is submitted.  The default since round 4 (ALFALFA_AMD_PACKED=0 /
    // aa_ctx_set_packed_coefficients( ctx, 0 ): dense blocks).
    bool packed = true;
    // One lane per DCT partition (tok_fsm.hh): frames with 2 / 4 / 8 partitions may be decoded by as many lanes of one wave.
    // Per context, fixed at the first submit (ALFALFA_AMD_LANE_PER_PARTITION=1 / aa_ctx_set_lane_per_partition).
    bool lane_per_partition = false;
    uint32_t mp_hint = 1;                // most partitions a frame submitted so far had (workgroups leave that many lanes per ticket)
    double words_per_byte = 4.0;         // running estimate for packed frames: 16-bit words stored per compressed byte
    uint32_t seen_starving = 0;
    std::vector<const uint32_t *> pending_lists;   // chunk lists of released frames, not yet handed to k_pool_free_lists
    // worker grids: slot g = worker stream g; counters are cumulative over the grids a slot has run
    static constexpr int kSlots = 8;
    struct Slot { hipStream_t st = nullptr; uint32_t launched = 0, gen = 0;
                  bool queued_behind_retiring = false;      // a grid was told to finish and a new one waits behind it on the stream ...
                  uint32_t retiring_until = 0; } slot[kSlots];  // ... until the slot's exit count reaches this (the old grid is gone)
    uint32_t * exited_dev = nullptr;     // [AA_MAX_WORKER_GRIDS] in HBM
    uint32_t * cu_slots_dev = nullptr;   // [AA_CU_SLOTS]: worker workgroups resident per CU (k_token_workers' admission; [last] = workgroups turned away)
    int cu_surplus = 0;                  // with the admission on: workgroups per CU a grid is launched with beyond what is wanted (ALFALFA_AMD_ADMISSION_SURPLUS)
    int cu_cap = -1;                     // worker workgroups a CU may hold (k_token_workers' admission): -1 = the shape's own number whenever the LDS request
                                         // would let one more in (the default), 0 = no admission, n = n (ALFALFA_AMD_CU_ADMISSION)
    unsigned long long * prof_dev = nullptr;   // diagnostics counters (ALFALFA_AMD_TOKEN_PROFILE=1), else null
    uint32_t * retire_host = nullptr, * retire_dev = nullptr;     // [AA_MAX_WORKER_GRIDS]: grids of generation <= this take no more jobs
    aa_tok_mirror * mirror_host = nullptr, * mirror_dev = nullptr;
    uint32_t mirror_seq = 0;
    hipEvent_t mirror_ev = nullptr;      // tok_peek_mirror: behind the refresh that is under way
    bool mirror_inflight = false;
    uint32_t lane_bytes = 0, lds = 0;
    int lanes = 0, cap_wgs = 0, n_cus = 0;
    // An idle wave stays this long before it leaves (100 MHz ticks; ALFALFA_AMD_WORKER_LINGER_MS).  100 ms: a wave that stays holds its
    // workgroup's 41 KB of LDS and its SIMD's wave slot against the reconstruction kernels for nothing; a wave that left costs a grid
    // launch when frames come again.  Measured on MI355X, round 5 (profiles/r05_bench_sessions.md, sessions 13/14, the driver's command):
    // 2 s -> 97.6-103.1 M macroblocks/s; 200 ms -> 114.6; 100 ms -> 117.7; 50 ms -> 118.4; 20 ms -> 116.3 (5-7 grids, 1 700-2 400
    // workgroups launched in the 20 steps instead of 1 grid of ~450) -- the drain above all: the last four steps take 0.6 s instead of 1.3
    unsigned long long linger_ticks = 10000000ull;
    // A top-up grid is launched when jobs wait and at least cap_wgs / this many workgroups are gone (ALFALFA_AMD_TOPUP_DIV).  An eighth:
    // with a quarter a 40-step run sat at 578 of 768 workgroups (just above the threshold) for twelve steps while the queue grew to
    // 6 700 jobs, and its drain then waited 1.5 s for the chains that started late (session 17); over 20 steps a quarter and an eighth
    // measure the same (117.8 M both, session 16), a sixteenth spends the worker streams on small grids.
    int topup_div = 8;
  } tok;
  // Device pieces given back while kernels that read them may still be queued: they become reusable once an event recorded
  // on the compute stream after the release has fired ("epochs": one event per group of releases, recorded lazily).
  struct PendingFree { uint8_t * p; size_t bytes; uint64_t epoch; };
  std::vector<PendingFree> pending_free;
  struct Epoch { uint64_t id; hipEvent_t compute, copy; };   // copy: null unless downloads were queued on the copy stream
  std::vector<Epoch> epoch_events;      // closed epochs, oldest first
  uint64_t open_epoch = 1;
  bool open_epoch_used = false;
  // Between the first raster binding of an aa_decode_batch call and its last launch no epoch may be closed: a raster that
  // bind_frame releases (an old reference, an output nobody holds) is still read or written by kernels that are not queued
  // yet, and an event recorded now would sit in FRONT of them on the compute stream.
  int binding_depth = 0;
  bool copy_reads_rasters = false;      // aa_stream_download_async queued copies since the last epoch was closed
  uint32_t stream_concurrency = 0, streams_needed = 0;    // probe_stream_concurrency (at the first submit)
  uint32_t clock_mhz = 0;                                 // hipDeviceAttributeClockRate, asked once
  bool profile = false;
  double host_share_ms = 80.0;
                                 // aa_submit_frames: a big call's key frames go to the host lanes while their backlog stays within this (0: never)
  int schedule = 0;            // 0: row-pipelined persistent kernels (default), 1: one launch per 2:1 anti-diagonal
  int n_xcd = 1;               // XCDs workgroups land on (probed at creation); row kernels keep a unit on one XCD
  int xcd_share[AA_MAX_XCD] = {};
  std::mutex pool_mu;           // pinned staging chunks given back by aa_stream_release_staging, reused by later parses
  std::vector<std::pair<uint8_t *, size_t>> pinned_pool;
  // Device memory of the streams (frame-store chunks, raster blocks) is carved out of 256-MiB slabs: allocation calls
  // serialise in the driver and hundreds of parser threads make them at once.  Freed pieces go to per-size free lists
  // (streams of one frame size all ask for the same two sizes); slabs are returned when the context dies.
  std::vector<uint8_t *> dev_slabs;
  uint8_t * cur_slab = nullptr;
  size_t slab_used = 0;
  size_t pool_bytes = 0;                  // HBM the pool has taken from HIP so far
  size_t pool_soft_limit = ~size_t( 0 );  // beyond this (slabs + mapped coefficient heap) the pool waits for released pieces rather than grow
                                          // (aa_ctx_create: 7/8 of what was free; aa_ctx_set_memory_limit)
  size_t pinned_bytes = 0;                // pinned host memory the context has taken (arenas, staging chunks, binding buffers)
  std::map<size_t, std::vector<uint8_t *>> dev_free;
  // Pieces whose every use -- by the old owner and by the next one -- is a kernel (or copy) queued on the COMPUTE stream: output
  // rasters and the transient dense coefficient blocks of a reconstruction call.  Stream order alone makes them reusable the
  // moment they are released (whatever still reads the old content was queued earlier on the same stream), so they do not wait
  // for a release epoch: a step releases ~45 GB of them at 1080p x 480 streams (a raster per frame, a dense piece per call),
  // which the epochs kept out of reach for one step -- 45 GB of pool that the coefficient heap could not have.  Only handed
  // out by dev_alloc_compute.  (A raster that a plain aa_stream_download_async may still be reading on the COPY stream takes the
  // epoch route: raster_download_pending.)
  std::map<size_t, std::vector<uint8_t *>> compute_free;
  size_t compute_free_bytes = 0;
  // ... released WHILE an aa_decode_batch call binds rasters (binding_depth > 0): the frame being bound still predicts from the
  // reference it has just let go of, and its kernels are not queued yet -- such a piece must not become another frame's output of
  // the same call.  It is held until the call's launches are queued (tests/test_gpu_parity.py::test_rasters_released_while_binding...).
  std::vector<std::pair<uint8_t *, size_t>> compute_hold;
  hipEvent_t last_raster_download = nullptr;   // recorded on the copy stream behind the last aa_stream_download_async
  bool raster_download_pending = false;
  uint64_t downloads_queued = 0, downloads_recorded = 0;   // aa_stream_download_async calls begun / whose event has been recorded (under pool_mu)
  std::mutex blank_mu;
  std::map<size_t, uint8_t *> blank;    // References( width, height ): one all-zero raster per raster size, shared by every new decoder (never written)
  uint8_t * boundary = nullptr; // loop filter: hand-off lines between macroblock rows (transient within a launch)
  size_t boundary_bytes = 0;
  aa_sync_ws * ws = nullptr;   // in-launch ordering state of the row-pipelined kernels
  size_t ws_bytes = 0;
  aa_kernel_stats stats {};
  struct Timed { hipEvent_t a, b; int kind; };
  std::vector<Timed> pending;
  std::vector<hipEvent_t> free_events;
};

namespace { void host_lanes_start( aa_ctx * ctx ); void host_lanes_stop( aa_ctx * ctx ); double host_lanes_rate( aa_ctx * ctx ); }
namespace { void hash_drain( aa_ctx * ctx ); void hash_free( aa_ctx * ctx ); }      // runtime_hashes.inc

struct aa_stream {
  aa_ctx * ctx;
  aa::Parser parser;
  uint8_t * dev_segmap = nullptr;   // persistent segment map in HBM (device-parsed frames), mb_width*mb_height bytes
  bool segmap_on_device = false;    // which copy is current: the parser's (host) or dev_segmap
  uint32_t pw, ph;
  size_t plane_bytes[3], slot_bytes;
  std::vector<Chunk> chunks;
  std::vector<Slot> slots;
  std::vector<FrameRec> frames;
  int cur_ref_slot[3];     // slot ids of last/golden/alt at PARSE time
  int cur_ref_frame[3];    // frame indices (for aa_stream_references)
  int next_submit = 0;     // device half progress
  int first_live = 0;      // frames below this index are fully released (aa_stream_release_before scans from here)
  aa_stream( aa_ctx * c, uint16_t w, uint16_t h ) : ctx( c ), parser( w, h ) {}
};
