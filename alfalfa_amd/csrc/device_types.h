// Records the HIP kernels read, as laid out in HBM.  Shared by runtime.cpp (host) and kernels.hip (device).
#pragma once
#include <stdint.h>

#include "../../include/alfalfa_amd.h"
#include "lf_choose.hh"

// One decoded-frame job, resident in HBM (one per (stream, frame)); built by the host when the frame is
// parsed: raster slots are assigned then (References bookkeeping = Frame::copy_to, frame.cc:271-307), so a
// job is self-contained and can be (re)played without touching the host.
struct aa_dev_frame {
  uint8_t * cur[3];            // output raster planes Y,U,V (padded, stride = padded width; raster.hh:54-56)
  const uint8_t * ref[4][3];   // [1] last, [2] golden, [3] altref planes ([0] unused)
  const aa_mb_info * mbs;      // mb_width*mb_height records
  const int16_t * coeffs;      // compact 16-coefficient blocks
  const unsigned long long * intra_rows;   // per MB row: ceil(mbw/64) words, bit c set = MB (c,row) is intra
  uint16_t quant[4][6];        // per segment {y_dc,y_ac,y2_dc,y2_ac,uv_dc,uv_ac}
  uint16_t mbw, mbh;
  uint8_t key_frame;
  uint8_t loop_filter_level;   // header value (0: no filtering at all)
  uint8_t sharpness;
  uint8_t has_intra;
  uint32_t packed;             // 1: packed coefficient storage (coeff_pack.hh) -- coeffs = the coefficient heap's base and a macroblock's record
                               // holds the offset of its words (reserved << 32 | coeff_index, in 16-bit words); 0: dense 16-coefficient blocks
};

// The raster planes of one frame job.  A job's records are final when the frame is parsed, but WHICH rasters it writes and
// predicts from is decided when it is handed to reconstruction (References bookkeeping, frame.cc:271-307): frames that are
// parsed far ahead of their decode -- the device parser keeps several batches in flight -- hold no raster until then.
struct aa_raster_binding {
  aa_dev_frame * job;
  uint8_t * cur[3];
  const uint8_t * ref[3][3];     // last, golden, altref
};

// One raster on its way out (aa_download_batch_async): `bytes` from `src` into piece i of the staging area
struct aa_gather_job {
  const uint8_t * src;
  size_t bytes;
};

// One frame on its way to RGB (aa_render_rgb_async): the display rectangle of a raster -> a caller's device buffer
struct aa_rgb_job {
  const uint8_t * plane[3];    // Y, U, V of the raster (padded planes)
  uint8_t * dst;               // row 0 (of plane 0 for CHW formats)
  int64_t row_stride, plane_stride;   // bytes
  uint32_t stride_y, stride_c; // padded widths of the luma and chroma planes
  uint32_t width, height;      // display size
  uint32_t groups;             // 16-pixel groups per row: (width + 15) / 16
  uint32_t pad;
};

// One plane of one pair on its way to a score (aa_quality_batch_async): a = the decoded plane, b = the original's
#define AA_QUALITY_STRIP_ROWS 8        // window rows per workgroup of k_quality_blocks
#define AA_QUALITY_CHUNK_WINDOWS 480   // ... and windows per row it holds; wider planes are cut into column chunks
struct aa_quality_job {
  const uint8_t * a, * b;
  int64_t stride_a, stride_b;  // bytes
  uint32_t w4, h4;             // 4x4 blocks per row and per column of the padded plane
  uint32_t groups;             // groups of four windows per window row: (w4 - 1 + 3) / 4
  uint32_t strips, chunks;     // workgroups: strips of AA_QUALITY_STRIP_ROWS window rows x column chunks
  uint32_t pad;
  uint64_t out_off;            // the plane's first group value in the workspace (floats; a multiple of 4)
};

// One (stream, new frame) of a rebase (aa_rebase_batch): the prediction frame's records, the references they predict from, the target
// planes, and where the forward path's results go.  The kernels read nothing else.
#define AA_REBASE_MB_BYTES ( 25 * 16 * 2 )   // dense coefficient scratch per macroblock: 25 slots (0..15 Y, 16..19 U, 20..23 V, 24 Y2) of 16 int16
struct aa_rebase_dev_job {
  const uint8_t * ref[4][3];   // [1] last, [2] golden, [3] altref planes of the job's stream ([0] unused)
  const uint8_t * target[3];   // padded, edge-extended planes the new frame stands for
  int64_t target_stride[2];    // bytes: luma, chroma
  uint8_t * recon[3];          // unfiltered reconstruction of the new frame (padded planes, stride = padded width): intra prediction reads it
  const aa_mb_info * mbs;      // mbw * mbh records of the prediction frame (modes, ref_frame, vectors, b_modes)
  int16_t * coeffs;            // [mbw * mbh][25][16]
  uint32_t * masks;            // [mbw * mbh]: bit b = slot b holds a non-zero coefficient
  uint16_t quant[6];           // {y_dc, y_ac, y2_dc, y2_ac, uv_dc, uv_ac} of the new frame
  uint16_t mbw, mbh;
  uint32_t has_intra;          // some macroblock is intra: the reconstruction is needed
  uint32_t pad;
};

// One (stream, new frame) of a rebase whose records stay in HBM (aa_rebase_device_batch), beside its aa_rebase_dev_job: where
// k_rebase_compact puts the frame -- the frame's own pool piece, laid out as a host-appended frame lies in its chunk -- and what the host
// knows of it beforehand: the job record (rasters unbound, pointers into the piece) and the intra-row words, both copied by the kernel.
struct alignas( 16 ) aa_rebase_compact_job {
  aa_dev_frame frame;                  // the template of *out_frame
  aa_dev_frame * out_frame;            // the piece's start
  aa_mb_info * out_mbs;                // mbw * mbh records
  int16_t * out_coeffs;                // num_coeff_blocks dense blocks
  unsigned long long * out_rows;       // rows_words words
  const unsigned long long * rows;     // ... as the host made them, in the slice's piece
  uint32_t rows_words;
  uint32_t num_coeff_blocks;           // the frame's blocks as the host summed them: nothing is stored at or beyond this block
};

// One (stream, new frame) of a re-encode (aa_reencode_batch): the rebase's job -- references, target, reconstruction, dense coefficient
// slots, masks, quantiser; mbs unused, has_intra 1 -- and what the decision adds: the job's rate model, the records it writes, and a
// side record per macroblock for the census and the B_PRED trial of its neighbours.
struct aa_reencode_dev_job {
  aa_rebase_dev_job base;
  const void * costs;          // aa::ReencCosts; a job of the forward encoder: aa::EncInterCosts or, a key frame, aa::EncKeyCosts (reencode_search.hh)
  aa_mb_info * mbs_out;        // mbw * mbh records: y_mode, uv_mode, ref_frame, nz_mask and u are the kernel's, the rest is zero
  uint32_t * nb;               // [mbw * mbh][4]: aa::ReencNeighbour
  unsigned long long * intra_rows;   // aa_reencode_device_batch: where k_reencode_count leaves the frame's intra-row words (else null, unused)
};

// One job of a size estimate (aa_estimate_size_batch, a round of aa_target_size_batch), beside its aa_reencode_dev_job over the SMALL frame:
// the tables the small frame's tokens are coded with and where k_estimate_tokens leaves its three words
struct aa_estimate_dev_job {
  const uint8_t * token_probs; // [4][8][3][11]: the stream's tables before the frame; a key estimate: the defaults
  uint32_t * result;           // [4]: the DCT partition's bytes, macroblocks with coefficients, intra macroblocks, 0
};

// One (stream, frame) of a serialisation (aa_serialize_batch): the frame's records as reconstruction reads them, the tables its tokens are
// coded with, and where the DCT partitions go: partition p owns [out + p * region, out + (p + 1) * region) and reports the bytes it takes
// -- more than `region`: it did not fit, and what did not fit was not stored -- in sizes[p].
struct aa_serialize_dev_job {
  const aa_dev_frame * frame;
  uint8_t * out;
  uint32_t * sizes;            // [8]
  uint32_t region;             // bytes per partition
  uint32_t nparts;             // 1, 2, 4 or 8
  uint32_t skip_enabled;       // the header has prob_skip_false: macroblocks flagged AA_MB_SKIP write no tokens
  uint32_t optimise;           // the probability passes run first: k_token_counts fills `counts`, k_token_probs turns `probs` (the tables before
                               // the frame) into the frame's tables and writes `updates`
  uint32_t * counts;           // [AA_SERIALIZE_COUNTS]: branch counts [4][8][3][11][2] {false, true}, then macroblocks with coefficients and
                               // macroblocks by reference frame (intra, last, golden, altref); zeroed by the host
  uint8_t * updates;           // [AA_SERIALIZE_UPDATES]: 1056 update flags, 1056 values, then prob_skip_false, prob_inter, prob_references_last,
                               // prob_references_golden as calc_prob gives them (0: no macroblock on the false side)
  uint8_t probs[1056];         // [4][8][3][11]
  const uint8_t * first_pass;  // (optimise) null, or [2112]: the update flags and values the FIRST pass of a two-pass key frame left; k_token_probs
                               // keeps them wherever this pass makes no update (the reference never clears the field between its passes)
};
#define AA_SERIALIZE_COUNTS ( 2112 + 8 )
#define AA_SERIALIZE_UPDATES ( 2112 + 8 )

// One job of a slice of the batched loop-filter level search (aa_lf_search_decode_batch), the same over all of its rounds: the frame's own
// job record (rasters bound: cur[] is the unfiltered reconstruction, three planes back to back; mbs its records) and where its candidates
// lie: candidate c of a round at cand + c * per, raster | records (records_off) | job record (job_off).
#define AA_LF_MAX_ROUND 8      // levels per job and round
struct aa_lf_search_dev_job {
  aa_dev_frame * frame;
  uint8_t * cand;
  uint64_t per;                // bytes
  uint32_t raster_bytes, luma_bytes, chroma_bytes;     // multiples of 16
  uint32_t records_off, job_off;
  uint32_t nmb;
  uint32_t pw, ph;             // the padded luma plane (measure 1 divides by it)
  int32_t level_hi;
  uint32_t pad;
  aa::LfSegments seg;          // the level of a macroblock by its segment (lf_choose.hh)
};
// One entry of a round's table: job `job` of the slice tries the levels first_level .. first_level + n - 1; their scores are
// [score_off, score_off + n) of the round's score arrays
struct aa_lf_round_entry { uint32_t job; int32_t first_level; uint32_t n; uint32_t score_off; };

#define AA_MAX_XCD 16

#define AA_SYNC_WS_DUMP 140
#define AA_SYNC_WS_RESCUES 132
// In-launch ordering state of the row-pipelined kernels; zeroed (hipMemsetAsync) before every such launch.
struct aa_sync_ws {
  int error;                   // != 0: a bounded spin expired (sticky; reported as AA_ERR_HIP by the host).  NOT zeroed per launch.
  int where[3];                // diagnostics of the FIRST expired wait: unit, row, need << 16 | seen
  int dump[AA_SYNC_WS_DUMP];   // ... and what that wave saw when it gave up: progress[] of every row of its unit (128), then polls, clock ticks waited, rows;
                               // [AA_SYNC_WS_RESCUES .. +2]: waits that only the slow path's second look ended (see reread_progress), by which of its reads
  int ticket[AA_MAX_XCD];      // per-XCD queue: next (unit,row) to hand out  -- zeroed from here on before every launch
  int progress[1];             // [unit in launch][mbh_max]: macroblock columns of that row that are final
};
#define AA_SYNC_WS_ZERO_FROM ( 16 + 4 * AA_SYNC_WS_DUMP )   // byte offset of `ticket`

#define AA_MAX_BATCH 480       // frames per launch and kind: kernel argument = 480 pointers (3840 B) passed by value (limit 4 KB)

struct aa_frame_list {
  const aa_dev_frame * f[AA_MAX_BATCH];
};

// one stream's share of a segment-map pass: its frames are order[first .. first+count) (bit 31 of an entry: the map restarts
// at all-3 with that frame), map = the stream's persistent segment map in HBM (mb_width*mb_height bytes)
struct aa_seg_stream { uint8_t * map; uint32_t first, count; };

// Counters of the device-side job queue / coefficient pool / worker grids as one kernel thread saw them, in pinned host memory
#define AA_MAX_WORKER_GRIDS 16
struct aa_tok_mirror {
  uint32_t seq;                // the mirror kernel's number (written last)
  uint32_t q_head, q_publish, q_reserve;
  int32_t pool_avail;
  uint32_t pool_starving;
  uint32_t exited[AA_MAX_WORKER_GRIDS];
  // diagnostics (ALFALFA_AMD_TOKEN_PROFILE=1), summed over the waves that have left, 100 MHz ticks: [0] boundary passes [1] their
  // number [2] wave steps [3] looking for / starting frames [4] ring top-ups [5] periods [6] lane-periods with a frame [7] periods
  unsigned long long prof[8];
};

// kernels.hip / parse_kernels.hip launchers (plain C++ signatures so runtime.cpp needs no HIP kernel syntax)
namespace aa {
struct ParseJob;   // tok_fsm.hh
struct TokQueue; struct CoeffPool; struct Heap;
// device-side entropy decode of n frames (jobs resident in HBM): macroblock headers, then (streams with segmentation only)
// the segment-map pass, then tokens
// order[slot] = job index: the host sorts the frames of a batch by chain length so that the lanes of a wave finish together
int launch_parse_mb_headers( const ParseJob * jobs, const uint32_t * order, int n, void * stream );
int launch_segment_fixup( const ParseJob * jobs, const aa_seg_stream * streams, int n_streams, const uint32_t * order, void * stream );
// token workers (tok_fsm.hh, parse_kernels.hip): lanes that take frames from a queue in HBM
void token_worker_shape( uint32_t lane_bytes, int n_cus, int * lanes_out, uint32_t * lds_out, int * wgs_per_cu_out );
int launch_token_workers( TokQueue * q, unsigned long long * slots, const Heap & heap, uint32_t * exited, const uint32_t * retire, uint32_t gen, uint32_t spread,
                          unsigned long long * prof, unsigned long long linger_ticks, int wgs, int lanes, uint32_t lane_bytes, uint32_t lds, bool packed, uint32_t mp_hint, void * stream,
                          uint32_t * cu_slots = nullptr, uint32_t cu_cap = 0 );
// (cu_slots: AA_CU_SLOTS counters in HBM, zero at start -- worker workgroups resident per CU, for the per-CU admission of k_token_workers)
#define AA_CU_SLOTS ( 16 * 256 )       /* (the upper half, but for its last word, is the token lanes' store sink: 8 KB nobody reads) */
int launch_enqueue_jobs( TokQueue * q, unsigned long long * slots, const ParseJob * jobs, const uint32_t * order, int n, void * stream );
int launch_pool_push_range( const Heap & heap, uint32_t first, uint32_t count, void * stream );
int launch_pool_free_lists( const Heap & heap, const uint32_t * const * lists, int n, void * stream );
int launch_mirror_counters( const TokQueue * q, const CoeffPool * pool, const uint32_t * exited, int n_grids, const unsigned long long * prof, aa_tok_mirror * out, uint32_t seq, void * stream );
// whole-vector inter macroblocks, four per wave
int launch_recon_inter4( const aa_frame_list & list, int n, unsigned max_mbs, void * stream );
// one inter macroblock per wave; split_only: only SPLITMV macroblocks (the rest is launch_recon_inter4's)
int launch_recon_inter( const aa_frame_list & list, int n, unsigned max_mbs, bool split_only, void * stream );
int launch_recon_intra_diagonal( const aa_frame_list & list, int n, int diagonal, int row_lo, int rows, void * stream );
int launch_loopfilter_diagonal( const aa_frame_list & list, int n, int diagonal, int row_lo, int rows, void * stream );
// Row kernels are XCD-affine: unit u (frame / group) is processed by workgroups that run on XCD u % n_xcd.
// list = groups of four frames of one geometry (slot 0 never null, missing frames null)
// list = groups of four frames (any geometry; slot 0 never null, missing frames null)
int launch_recon_intra4( const aa_frame_list & list, int n_groups, int mbh_max, aa_sync_ws * ws, int n_xcd, void * stream );
// boundary: 128 bytes per (frame slot of the list, MB row, MB column) = 4 * n_groups * mbh_max * mbw_max lines; transient
int launch_loopfilter_rows4( const aa_frame_list & list, int n_groups, int mbh_max, int mbw_max, aa_sync_ws * ws, uint8_t * boundary, int n_xcd, void * stream );
// out16[x] += number of workgroups (of `blocks`) that ran on XCD x
int launch_probe_xcds( int * out16, int blocks, void * stream );
// seen[slot] = how many of the n probe kernels (one per stream) had arrived when this one gave up waiting or all were there
int launch_probe_concurrency( uint32_t * counter, uint32_t * seen, uint32_t n, unsigned long long timeout_ticks, int slot, void * stream );
int launch_bind_rasters( const aa_raster_binding * b, int n, void * stream );
// raster i (jobs[i]) -> staging + i * stride, one launch for the lot
int launch_gather_rasters( const aa_gather_job * jobs, int n, uint8_t * staging, size_t stride, size_t max_bytes, void * stream );
// jobs[i] -> RGB in `format` (AA_RGB_*), one launch for the lot; table: 3 x 256 output values (float formats); max_threads: the largest
// job's groups * row pairs
int launch_render_rgb( const aa_rgb_job * jobs, int n, int format, const uint32_t * table, uint32_t max_threads, void * stream );
// dst = src with lf_level := byte `segment_id` of `levels` (records are 80 bytes, 16-byte aligned)
int launch_lf_relevel( const aa_mb_info * src, aa_mb_info * dst, unsigned nmb, uint32_t levels, void * stream );
// lf_search_kernels.hip (see there): a round's candidates -- rasters, re-levelled records, job records -- from its table; the rule continued over
// the round's scores (measure 0: ssim; 1: made from sse); the chosen level into every job's own records and job record
int launch_lf_candidates( const aa_lf_search_dev_job * jobs, const aa_lf_round_entry * entries, int n_entries, uint32_t max_raster_bytes, void * stream );
int launch_lf_choose( const aa_lf_search_dev_job * jobs, const aa_lf_round_entry * entries, int n_entries, const double * ssim, const unsigned long long * sse, int measure,
                      LfChoice * states, void * stream );
int launch_lf_finish( const aa_lf_search_dev_job * jobs, const LfChoice * states, int n_jobs, uint32_t max_mbs, void * stream );
// hash_kernels.hip: job i (hash_chain.hh; n of them, longest first) is walked by lane i % lanes_per_wave of wave i / lanes_per_wave; its
// result goes to results[job.out_index] (out_index < n)
struct HashJob;
int launch_hash_chains( const HashJob * jobs, int n, int lanes_per_wave, uint64_t * results, void * stream );
// quality_kernels.hip: jobs[i] (n_planes of them) -> ssim[i], sse[i] (optional; zeroed by the caller): k_quality_blocks over
// max_blocks x n_planes workgroups (max_blocks: the largest job's strips * chunks), then k_quality_sum; group_values: the workspace
int launch_quality( const aa_quality_job * jobs, int n_planes, uint32_t max_blocks, float * group_values, double * ssim, unsigned long long * sse, void * stream );
// rebase_kernels.hip: jobs[i] (n of them; max_mbs: the largest job's macroblocks) -> dense coefficients, masks and the unfiltered
// reconstruction: k_rebase_inter over every inter macroblock, then (any_intra) k_rebase_intra, one wave per job
int launch_rebase( const aa_rebase_dev_job * jobs, int n, uint32_t max_mbs, bool any_intra, void * stream );
// rebase_compact_kernels.hip, behind launch_rebase on the same stream: k_rebase_count leaves the stored blocks of run r (256 macroblocks)
// of job i in partials[i * stride + r] (stride >= the largest job's runs); k_rebase_compact, given the frames' pieces (outs[i]), writes
// records, dense blocks in parse order, job record and intra-row words there
int launch_rebase_count( const aa_rebase_dev_job * jobs, int n, uint32_t max_mbs, uint32_t * partials, uint32_t stride, void * stream );
int launch_rebase_compact( const aa_rebase_dev_job * jobs, const aa_rebase_compact_job * outs, int n, uint32_t max_mbs, const uint32_t * partials, uint32_t stride, void * stream );
// reencode_kernels.hip: jobs[i] (n of them) -> records, dense coefficients, masks and the unfiltered reconstruction: k_reencode_inter, one
// workgroup per job; slots: macroblocks of an anti-diagonal a round takes (1..16)
int launch_reencode( const aa_reencode_dev_job * jobs, int n, int slots, void * stream );
// encode_kernels.hip: the same over jobs of ONE kind of the forward encoder -- key: k_encode_key (costs = EncKeyCosts, no reference read),
// otherwise k_encode_inter (costs = EncInterCosts)
int launch_encode( const aa_reencode_dev_job * jobs, int n, bool key, int slots, void * stream );
// a two-pass key job behind its first pass: k_key2_first_pass, k_key2_updates, k_encode_key2 (encode_two_pass_kernels.hip)
int launch_encode_second_pass( const aa_reencode_dev_job * jobs, int n, uint32_t max_mbs, int slots, void * stream );
// estimate_kernels.hip: the same over jobs of ONE kind of the size estimate, whose frames are the small ones -- key: k_estimate_key (costs =
// EstKeyCosts), otherwise k_estimate_inter (costs = EstInterCosts) -- and, behind them on the same stream, k_estimate_tokens: a lane per job,
// lanes_per_wave (1..64) to a wave, sizes[i] beside jobs[i]
int launch_estimate( const aa_reencode_dev_job * jobs, int n, bool key, int slots, void * stream );
int launch_estimate_tokens( const aa_reencode_dev_job * jobs, const aa_estimate_dev_job * sizes, int n, int lanes_per_wave, void * stream );
// reencode_compact_kernels.hip, behind launch_reencode on the same stream: the pair of launch_rebase_count / launch_rebase_compact over the
// records the decision wrote.  k_reencode_count also leaves every frame's intra-row words in jobs[i].intra_rows; k_reencode_compact copies
// them from there (outs[i].rows) and sets lf_level by lf[i] (aa::HeaderParams, n of them)
int launch_reencode_count( const aa_reencode_dev_job * jobs, int n, uint32_t max_mbs, uint32_t * partials, uint32_t stride, void * stream );
int launch_reencode_compact( const aa_reencode_dev_job * jobs, const aa_rebase_compact_job * outs, const void * lf, int n, uint32_t max_mbs, const uint32_t * partials, uint32_t stride,
                             void * stream );
// serialize_kernels.hip: k_serialize_tokens, a lane per (job, DCT partition): lanes[i] = job << 3 | partition, n_lanes of them,
// lanes_per_wave (1..64) to a wave
int launch_serialize_tokens( const aa_serialize_dev_job * jobs, const uint32_t * lanes, int n_lanes, int lanes_per_wave, void * stream );
// ... the probability passes in front of it, for the jobs (of n) that have `optimise` set: k_token_counts over runs of macroblocks x jobs
// (max_mbs: the largest job's macroblocks), then k_token_probs, a thread per job and probability
int launch_serialize_probs( aa_serialize_dev_job * jobs, int n, uint32_t max_mbs, void * stream );
}
