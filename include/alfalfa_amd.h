/* alfalfa_amd.h -- C ABI of the MI355X-native VP8 decode hot path (drop-in for excamera/alfalfa src/decoder).
 *
 * The reference has no FFI layer: its seam is the C++ class API Decoder / DecoderState / References /
 * RasterHandle / VP8Raster (decoder.hh:123-300, raster_handle.hh:77-123, vp8_raster.hh:53-316).  This
 * header is the plain-C boundary underneath our C++ mirror of those classes (include/alfalfa_amd/ C++ headers)
 * and underneath any other binding (ctypes in alfalfa_amd/capi.py).  Plain pointers
 * and sizes only; every function returns an aa_status and never throws.  No torch types.
 *
 * Pipeline (reference call stack SURVEY.md 3.1):
 *   host   aa_parser_*      decompress_frame + parse_frame  (uncompressed_chunk.cc:34-155, decoder_state.hh:72-167,
 *                           frame.cc:95-137, macroblock.cc:43-502, tokens.cc:50-135) -> macroblock records + coefficient blocks
 *   device aa_stream_*      decode_frame: Frame::decode + Frame::loopfilter + Frame::copy_to (decoder.cc:101-118,
 *                           frame.cc:139-307) as HIP kernels over device-resident rasters
 *   batch  aa_decode_batch  one pass of the hot path over frame f_i of N independent streams (ExCamera chunks / GOPs)
 *
 * There is NO CPU fallback for the device half: without a HIP device every aa_ctx_* / aa_stream_* call fails
 * with AA_ERR_NO_DEVICE.  The parser half is host code by design (serial BoolDecoder) and runs anywhere.
 */
#ifndef ALFALFA_AMD_H
#define ALFALFA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (round 5): aa_ctx_info and aa_kernel_stats grew in round 4 (a caller built against version 3 passes smaller structs: check
 * aa_abi_version() against the header you compiled with before calling aa_ctx_get_info / aa_ctx_kernel_stats), packed coefficient
 * storage became the default, AA_SUBMIT_HOST on a big call no longer waits for the parse (host lanes), hand-overs are refused at the memory limit.
 * Still 4 with the serialisation (aa_frame_header_ext, aa_parser_last_header_ext / aa_stream_last_header_ext, aa_parser_last_sub_modes /
 * aa_stream_last_sub_modes, aa_serialize_batch, aa_serialize_last_timing): those are additions -- new entry points and new structs, no
 * existing struct, enum or call changed -- so a caller built against version 4 is served as before; a caller that wants them asks the
 * library for the symbols (dlsym / the bindings' symbol table), as tests/test_serialize_abi.py does. */
#define AA_ABI_VERSION 4

typedef enum aa_status {
  AA_OK = 0,
  AA_ERR_INVALID = -1,      /* reference: Invalid("invalid bitstream: ...")       exception.hh:76-82  */
  AA_ERR_UNSUPPORTED = -2,  /* reference: Unsupported("unsupported bitstream: ...") exception.hh:84-90 */
  AA_ERR_LOGIC = -3,        /* reference: LogicError                                exception.hh:92-98  */
  AA_ERR_OUT_OF_RANGE = -4, /* reference: std::out_of_range from Chunk bounds       chunk.hh:54-59     */
  AA_ERR_HIP = -5,          /* HIP runtime failure (message has hipGetErrorString)                      */
  AA_ERR_NO_DEVICE = -6,    /* no HIP device / kernels missing: the device path NEVER falls back to CPU */
  AA_ERR_ARGUMENT = -7,
  AA_ERR_NO_MEMORY = -8     /* HBM: the memory limit of the context leaves no room (the message says what to release); the call can be repeated */
} aa_status;

/* Message of the last failing call on this thread ("" if none). */
const char * aa_last_error( void );
int aa_abi_version( void );
/* The HIP runtime reads GPU_MAX_HW_QUEUES when it starts; this library runs 16 HIP streams side by side (long-lived entropy-decode
 * grids beside short reconstruction kernels) and wants 16 hardware queues (the default is 4).  Call this before the process makes
 * its first HIP call -- the bindings call it before their first aa_ctx_create -- to set the variable if the environment does not
 * (a value that is set stands).  -> 1 if it was set already, 0 if this call set it.  Nothing else of the host process is touched;
 * a context checks what it really got (aa_ctx_info::stream_concurrency). */
int aa_runtime_prepare( void );
/* Cores this process can really use: hardware threads and affinity mask bounded by the cgroup CPU quota (a container may show 256
 * and grant 16).  The host workers of aa_submit_frames are never more than twice this, whatever `threads` says. */
int aa_host_cpus( void );
/* Number of visible HIP devices (0 when there is none; never fails). */
int aa_device_count( void );

/* ------------------------------------------------------------------------------------------------
 * Parsed-frame records (what Appendix B of SURVEY.md says the device needs).  Layout is ABI.
 * ---------------------------------------------------------------------------------------------- */

/* Per-macroblock record, 80 bytes.  Modes use the reference's enums (modemv_data.hh:37-49). */
typedef struct aa_mb_info {
  uint8_t y_mode;        /* mbmode: DC_PRED,V_PRED,H_PRED,TM_PRED,B_PRED,NEARESTMV,NEARMV,ZEROMV,NEWMV,SPLITMV */
  uint8_t uv_mode;       /* DC_PRED..TM_PRED (intra MBs) */
  uint8_t ref_frame;     /* reference_frame: 0 CURRENT (intra), 1 LAST, 2 GOLDEN, 3 ALTREF */
  uint8_t segment_id;    /* 0..3 (persistent map value; 0 when segmentation is off) */
  uint8_t flags;         /* AA_MB_* */
  uint8_t lf_level;      /* final loop-filter level of this MB, 0 = not filtered, else 1..63
                            (segment + ref + mode adjustments applied, loopfilter.cc:43-79, macroblock.cc:611-623) */
  uint8_t split_partition; /* SPLITMV partition id (mv_partitions index) */
  uint8_t reserved;
  uint32_t nz_mask;      /* bit b set: block b has stored coefficients. b: 0..15 Y (raster), 16..19 U, 20..23 V, 24 Y2.
                            Stored blocks follow each other in PARSE order: Y2 (if bit 24), then bits 0..23 ascending */
  uint32_t coeff_index;  /* index (in 16-coefficient blocks) of this MB's first stored block in the frame's coefficient array */
  union {
    uint8_t b_mode[16];  /* B_PRED: bmode of each 4x4 (intra MBs) */
    int16_t mv[16][2];   /* inter MBs: {x, y} of each Y sub-block, quarter-pel (all equal unless SPLITMV) */
  } u;
} aa_mb_info;

#define AA_MB_HAS_NONZERO 1u   /* Macroblock::has_nonzero_: residual path runs (macroblock.cc:531,547,579,593) */
#define AA_MB_HAS_Y2 2u        /* Y2 coded: mode is neither B_PRED nor SPLITMV (block.hh:183-190) */
#define AA_MB_INTER 4u         /* inter_coded() */
#define AA_MB_SKIP 8u          /* mb_skip_coeff */
#define AA_MB_LF_SKIP_INNER 16u /* loop filter skips sub-block edges: Y2 coded && !has_nonzero (macroblock.cc:607) */

/* Per-frame constants. */
typedef struct aa_frame_header {
  uint8_t key_frame, show_frame;
  uint8_t loop_filter_level;   /* header value; 0 => Frame::loopfilter is skipped entirely (frame.cc:143) */
  uint8_t sharpness_level;
  uint8_t num_dct_partitions;
  uint8_t segmentation_enabled, filter_adjustments_enabled;
  uint8_t refresh_last, refresh_golden, refresh_alternate;  /* key frames: all 1 */
  uint8_t copy_buffer_to_golden, copy_buffer_to_alternate;  /* 0 none, 1 last, 2 the other (frame.cc:278-292) */
  uint8_t sign_bias_golden, sign_bias_alternate;
  uint8_t q_index;
  uint8_t has_intra_mb;        /* any intra MB in this frame (always 1 for key frames) */
  uint16_t mb_width, mb_height;
  uint16_t width, height;      /* display size */
  /* dequantisation factors per segment (index 0 used when segmentation is off; all 4 filled):
     {y_dc, y_ac, y2_dc, y2_ac, uv_dc, uv_ac}  quantization.cc:83-93, frame.cc:185-206 */
  uint16_t quant[4][6];
  uint32_t num_macroblocks;
  uint32_t num_coeff_blocks;   /* stored 16-coefficient blocks (32 bytes each) */
  uint32_t num_intra_mbs;
  uint32_t compressed_size;
} aa_frame_header;

/* What the frame header of the bitstream holds beyond aa_frame_header (frame_header.hh:194-295): the fields a decoder consumes while it
 * parses and a serialiser has to write (serializer.cc:110-181).  A `*_update[i]` byte says that the Flagged<> entry is present; the value
 * beside it is what the bitstream holds (zero when absent).  aa_parser_last_header_ext / aa_stream_last_header_ext return the struct of
 * the frame just parsed; aa_serialize_batch takes one per job.  Layout is ABI (bytes only). */
typedef struct aa_frame_header_ext {
  uint8_t color_space, clamping_type;                    /* key frames (the decoder refuses a frame that sets either) */
  uint8_t filter_type;                                   /* 1: the 'simple' loop filter (refused by the decoder) */
  uint8_t refresh_entropy_probs;
  /* UpdateSegmentation (present when aa_frame_header::segmentation_enabled) */
  uint8_t update_mb_segmentation_map, update_segment_feature_data, segment_feature_mode /* 1: absolute values */;
  uint8_t lf_delta_update;                               /* ModeRefLFDeltaUpdate present (with filter_adjustments_enabled) */
  uint8_t seg_quant_update[4]; int8_t seg_quant[4];      /* quantizer_update: 7 bits + sign */
  uint8_t seg_lf_update[4]; int8_t seg_lf[4];            /* loop_filter_update: 6 bits + sign */
  uint8_t seg_tree_update[3], seg_tree_probs[3];         /* mb_segmentation_map (with update_mb_segmentation_map); absent = 255 */
  uint8_t skip_enabled, prob_skip_false;                 /* Flagged prob_skip_false */
  uint8_t ref_lf_update[4]; int8_t ref_lf_delta[4];      /* ref_update: 6 bits + sign */
  uint8_t mode_lf_update[4]; int8_t mode_lf_delta[4];    /* mode_update */
  uint8_t q_update[5]; int8_t q_delta[5];                /* y_dc, y2_dc, y2_ac, uv_dc, uv_ac: 4 bits + sign */
  uint8_t prob_inter, prob_references_last, prob_references_golden;   /* inter frames */
  uint8_t intra_16x16_update, intra_16x16_prob[4];
  uint8_t intra_chroma_update, intra_chroma_prob[3];
  uint8_t mv_prob_update[2][19], mv_prob[2][19];         /* the 7 bits written: the table entry becomes x ? x << 1 : 1 */
  uint8_t token_prob_update[4][8][3][11], token_prob[4][8][3][11];
} aa_frame_header_ext;

/* ------------------------------------------------------------------------------------------------
 * Host parser: the reference's DecoderState + parse_frame (decoder_state.hh:72-167).  Host only.
 * ---------------------------------------------------------------------------------------------- */
typedef struct aa_parser aa_parser;

aa_status aa_parser_create( uint16_t width, uint16_t height, aa_parser ** out );
void aa_parser_destroy( aa_parser * p );

/* Parse one compressed frame (Chunk = {data,size}, chunk.hh:38-73) and apply it to the persistent state.
 * mb_out must hold mb_width*mb_height records; coeff_out must hold 25*16*mb_width*mb_height int16 (worst case).
 * On error the persistent state is left as the reference leaves it (it may already be modified). */
aa_status aa_parser_parse( aa_parser * p, const uint8_t * data, size_t size,
                           aa_frame_header * hdr_out, aa_mb_info * mb_out, int16_t * coeff_out );

/* Decoder::set_error_concealment (decoder.hh:298; FramePlayer::set_error_concealment player.hh:72; salsify-receiver.cc:192): a frame
 * that ends inside its first partition, or before its tag is complete, is ACCEPTED (UncompressedChunk accept_partial,
 * uncompressed_chunk.cc:34-130) -- what is there of the first partition is used, decoders read zeros past the end, a frame
 * without a complete tag becomes an inter frame of no bytes -- instead of AA_ERR_INVALID.  Off by default, as in the reference. */
aa_status aa_parser_set_error_concealment( aa_parser * p, int on );
/* The rest of the header of the frame this parser parsed last (aa_parser_parse; all zero before the first). */
aa_status aa_parser_last_header_ext( const aa_parser * p, aa_frame_header_ext * out );
/* ... and what its records do not hold: a SPLITMV macroblock's record has every partition's VECTOR, not the sub-block mode (10 LEFT4X4, 11
 * ABOVE4X4, 12 ZERO4X4, 13 NEW4X4) that said it.  out[0 .. *count): the modes of the frame parsed last, partition after partition in bitstream
 * order; out may be NULL (count only); more than `capacity` entries: AA_ERR_ARGUMENT, *count still set.  A serialiser that is to write the
 * frame's own bytes back needs them (aa_serialize_job::sub_modes). */
aa_status aa_parser_last_sub_modes( const aa_parser * p, uint8_t * out, size_t capacity, size_t * count );
/* UncompressedChunk( frame, expected_width, expected_height, accept_partial ) (uncompressed_chunk.cc:34-130): what the frame tag
 * says, with the reference's checks and error classes.  corruption_level: 0 NO_CORRUPTION, 2 CORRUPTED_FIRST_PARTITION,
 * 3 CORRUPTED_FRAME (uncompressed_chunk.hh:40-46).  Any out pointer may be NULL. */
aa_status aa_parse_frame_tag( const uint8_t * data, size_t size, uint16_t width, uint16_t height, int accept_partial,
                              int * key_frame, int * show_frame, int * experimental, int * corruption_level );

/* Persistent state (DecoderState, decoder.hh:190-225), flat export for tests / serialisation:
 * probs[1101] = 1056 coefficient, 4 y-mode, 3 uv-mode, 38 mv probabilities. */
aa_status aa_parser_get_probs( const aa_parser * p, uint8_t probs[1101] );
/* segmentation: enabled, absolute, quant[4], lf[4]; map (mb_width*mb_height bytes) may be NULL */
aa_status aa_parser_get_segmentation( const aa_parser * p, int * enabled, int * absolute, int8_t quant[4], int8_t lf[4], uint8_t * map );
aa_status aa_parser_get_filter_adjustments( const aa_parser * p, int * enabled, int8_t ref[4], int8_t mode[4] );

/* DecoderState as one flat blob: the host half of the entry-state hand-off `Decoder( DecoderState, References )`
 * (decoder.cc:43-46; the device half is aa_stream_import_reference).  Size depends only on the frame size. */
size_t aa_parser_state_size( const aa_parser * p );
aa_status aa_parser_export_state( const aa_parser * p, uint8_t * buf, size_t capacity );
aa_status aa_parser_import_state( aa_parser * p, const uint8_t * buf, size_t size );

/* The same state in the REFERENCE's wire format: DecoderState::serialize / DecoderState::deserialize
 * (decoder.cc:283-330; tags and little-endian integers of enc_state_serializer.hh:43-86).  buf == NULL: size query. */
aa_status aa_parser_serialize_state( const aa_parser * p, uint8_t * buf, size_t capacity, size_t * size );
aa_status aa_parser_deserialize_state( aa_parser * p, const uint8_t * buf, size_t size );

/* ------------------------------------------------------------------------------------------------
 * Device context: one per GPU (one process per GPU in multi-GPU runs).
 * ---------------------------------------------------------------------------------------------- */
typedef struct aa_ctx aa_ctx;
typedef struct aa_stream aa_stream;

aa_status aa_ctx_create( int device, aa_ctx ** out );
void aa_ctx_destroy( aa_ctx * ctx );
aa_status aa_ctx_sync( aa_ctx * ctx );               /* waits for copy + compute streams */
/* HBM of the context's device: bytes free / total right now (hipMemGetInfo).  Either pointer may be NULL. */
aa_status aa_ctx_memory( aa_ctx * ctx, size_t * free_bytes, size_t * total_bytes );
/* Launch schedule of the dependency-ordered kernels (intra prediction, loop filter):
 *   AA_SCHEDULE_ROWS (default)  row-pipelined persistent kernels, rows ordered in-launch by ticket + progress words
 *   AA_SCHEDULE_DIAGONAL        one launch per 2:1 anti-diagonal (kernel boundary = synchronisation); for A/B runs
 * Also selectable with the environment variable ALFALFA_AMD_SCHEDULE=rows|diagonal at context creation. */
#define AA_SCHEDULE_ROWS 0
#define AA_SCHEDULE_DIAGONAL 1
aa_status aa_ctx_set_schedule( aa_ctx * ctx, int schedule );
/* The row-pipelined kernels keep a sticky error word (a bounded in-launch wait expired, a wave migrated between XCDs, a
 * ticket queue was not drained): once set, aa_ctx_sync / downloads report AA_ERR_HIP and later launches give up early.
 * After the caller has dealt with it (e.g. switched to AA_SCHEDULE_DIAGONAL), this clears the word. */
aa_status aa_ctx_clear_error( aa_ctx * ctx );
/* HBM the context may take for its pools (frame records, rasters, the coefficient heap of the device parser): by default 7/8 of
 * what was free when it was created; a caller that shares the GPU sets less.  Memory is taken as frames need it, up to this.
 * Round 5: the limit bounds what the context ACCEPTS.  aa_submit_frames stops a thirty-second short of it: a hand-over whose
 * arena would take pool + mapped coefficient heap beyond that first waits for pieces released behind queued kernels, and when
 * none are left is refused with AA_ERR_NO_MEMORY (nothing is appended; repeatable once frames have been reconstructed and
 * released) -- a pipelining caller treats that as "not now".  The coefficient heap, which never unmaps, leaves a sixteenth of
 * the limit to the pool.  Reconstruction (rasters, transient dense blocks) is never refused: it lives on what is kept back, and
 * goes past the limit only if the caller holds more decoded frames at once than that covers. */
aa_status aa_ctx_set_memory_limit( aa_ctx * ctx, size_t bytes );
/* What the context holds right now (the memory budget of a deployment: one context per GPU, one process per GPU). */
typedef struct aa_ctx_info {
  uint64_t memory_limit_bytes;       /* aa_ctx_set_memory_limit */
  uint64_t pool_bytes;               /* HBM taken for frame records, rasters, batch arenas (slabs, recycled) */
  uint64_t pool_free_bytes;          /* ... of which in the free lists right now */
  uint64_t pool_pending_bytes;       /* ... of which released but possibly still read by queued kernels */
  uint64_t heap_mapped_bytes;        /* HBM mapped into the coefficient heap of the device parser */
  uint64_t heap_limit_bytes;         /* its virtual size */
  uint64_t heap_used_bytes;          /* chunks frames hold or are expected to take */
  uint64_t pinned_host_bytes;        /* pinned host memory (batch arenas, staging chunks) */
  uint32_t heap_is_virtual;          /* 1: grown on demand (hipMemMap); 0: one fixed allocation (no virtual memory management) */
  uint32_t token_lanes_per_workgroup, token_workgroups_capacity, token_workgroups_alive;
  uint32_t token_lane_lds_bytes, token_workgroup_lds_bytes;
  uint32_t jobs_waiting;             /* frames in the token workers' queue that no lane has taken */
  uint32_t compute_units;
  int32_t heap_free_chunks;          /* 64-KB chunks in the coefficient pool */
  uint32_t lanes_starved;            /* times a token lane found the pool empty (since the context was created) */
  /* diagnostics, ALFALFA_AMD_TOKEN_PROFILE=1 (else zero): where the token workers' waves spent their time, summed over the waves
   * that have left, in 10-ns ticks: [0] macroblock-boundary passes [1] how many [2] decode steps of waves [3] looking for /
   * starting frames [4] ring top-ups [5] periods (steps + boundary passes) [6] lane-periods that had a frame [7] periods */
  uint64_t token_profile[8];
  uint32_t packed_coefficients;      /* 1: device-parsed frames store packed coefficients (aa_ctx_set_packed_coefficients) */
  uint32_t lane_per_partition;       /* 1: frames with several DCT partitions may get a token lane per partition (aa_ctx_set_lane_per_partition) */
  uint32_t clock_mhz;                /* the device's shader clock (hipDeviceAttributeClockRate) */
  uint32_t host_share_ms;            /* aa_ctx_set_host_share_ms */
  uint32_t host_rate_kb_per_ms;      /* what the host lanes get through, all workers together (KB of compressed data per ms: measured on the frames they have parsed,
                                        parse time only; 0: none yet).  The share of later calls is planned with it: visible cores and usable cores differ under a CPU quota */
  uint32_t reserved1;
  uint32_t stream_concurrency;       /* how many of the context's HIP streams were seen running side by side (probed at the first aa_submit_frames; 0: not yet) */
  uint32_t streams_needed;           /* ... of how many (16): fewer means GPU_MAX_HW_QUEUES was not in effect, see aa_runtime_prepare */
  uint32_t host_waited_parse_ms;     /* aa_decode_batch waiting for the device parser, since the last aa_ctx_kernel_stats reset (= its parse_wait_ms, without its synchronisation) */
  uint32_t host_waited_compute_ms;   /* ... for a raster-binding buffer: the compute stream was 16 calls behind (= bind_wait_ms) */
} aa_ctx_info;
aa_status aa_ctx_get_info( aa_ctx * ctx, aa_ctx_info * out );
/* How the device parser stores a frame's coefficients until the frame is reconstructed.  1 (default): packed -- per macroblock 25
 * mask slots + the non-zero coefficients in parse order (about a third of the memory on video content, and fewer stores for the
 * token lanes); the reconstruction kernels read that form themselves (since round 6: no dense copy is made).
 * 0: dense, 32 bytes per non-zero 4x4 block.  Results are identical.  The choice is per context and can only be made before
 * the context's first aa_submit_frames call (AA_ERR_LOGIC afterwards); the environment variable ALFALFA_AMD_PACKED=0 makes
 * dense the default of every context. */
aa_status aa_ctx_set_packed_coefficients( aa_ctx * ctx, int on );
/* Key frames of big calls on the host's cores.  aa_submit_frames hands a call with many streams to the GPU's token lanes; a KEY
 * frame's chain is the longest there is (seconds on a lane, ~35 ms on a core) and its group cannot be reconstructed before it
 * is parsed, so the streams of such a call whose frames are all key frames go to the context's host lanes instead (see
 * AA_SUBMIT_HOST: the same records, and the call does not wait) -- biggest first, while what the host lanes have been given and
 * not finished stays within `ms` milliseconds of their work at the rate they have really achieved.  Default 80 (environment:
 * ALFALFA_AMD_HOST_SHARE_MS); 0: every frame of a big call goes to the GPU's lanes.  AA_SUBMIT_DEVICE overrides it per call. */
aa_status aa_ctx_set_host_share_ms( aa_ctx * ctx, double ms );
/* One token lane per DCT partition.  A frame with 2, 4 or 8 partitions (frame.cc:119-137: macroblock row r is coded in
 * partition r % P) is then decoded by that many lanes of one wave -- rows handed from lane to lane through the above-row
 * flags in LDS --, whenever the wave that draws it has the lanes idle; its entropy-decode latency falls towards 1 / P of the
 * single-lane figure.  Single-partition frames, records and rasters are unaffected.  Per context, before its first
 * aa_submit_frames call (AA_ERR_LOGIC afterwards); ALFALFA_AMD_LANE_PER_PARTITION=1 makes it the default.  Off by default:
 * simulated on the host lane by lane and wave by wave (tests/test_wave_sim.py) and run on the GPU (tests/test_gpu_lane_per_partition.py). */
aa_status aa_ctx_set_lane_per_partition( aa_ctx * ctx, int on );
/* hipStream_t handles as opaque pointers (to order foreign work, e.g. an RCCL broadcast, against ours) */
void * aa_ctx_compute_stream( aa_ctx * ctx );
void * aa_ctx_copy_stream( aa_ctx * ctx );

/* ------------------------------------------------------------------------------------------------
 * Stream decoder: the reference's Decoder (decoder.hh:244-300) with device-resident References.
 * Frames are appended in bitstream order; rasters live in HBM and are fetched on demand.
 * ---------------------------------------------------------------------------------------------- */
aa_status aa_stream_create( aa_ctx * ctx, uint16_t width, uint16_t height, aa_stream ** out );
void aa_stream_destroy( aa_stream * s );

/* Host half: parse frame into pinned staging (no GPU work). Returns the frame's index in *frame_index. */
aa_status aa_stream_parse( aa_stream * s, const uint8_t * data, size_t size, int * frame_index, aa_frame_header * hdr_out );
/* Append a frame given as RECORDS -- header (quantiser factors, loop-filter level, reference update flags ...), macroblock records
 * with their final loop-filter levels, coefficient blocks in parse order -- instead of as a bitstream: the reference update of
 * Encoder::write_frame (encoder.cc:146-160: frame.decode + frame.loopfilter + copy_to on a Frame the encoder holds) and the replay
 * of xc-enc -r (frontend/xc-enc.cc:286-300) need no serialise -> parse round trip.  The records are what aa_parser_parse /
 * aa_stream_read_records produce.  The stream's DecoderState is NOT advanced (it belongs to whoever made the records); the frame
 * is decoded by aa_decode_batch like any other. */
aa_status aa_stream_append_records( aa_stream * s, const aa_frame_header * hdr, const aa_mb_info * mbs, const int16_t * coeffs, int * frame_index );
/* hipMemcpyAsync (copy stream) of every parsed, not yet uploaded frame's records into HBM. */
aa_status aa_stream_upload( aa_stream * s );
/* Give the pinned host staging of everything uploaded so far back to the system (the device copy is what decode reads).
 * Waits for this context's copy stream.  Later aa_stream_parse calls stage into fresh pinned memory.  Optional: a
 * long-lived bundle decoder that parses ahead of decoding calls it to bound pinned memory. */
aa_status aa_stream_release_staging( aa_stream * s );
/* Device half for frame `frame_index` of each of n streams (all on the same ctx): reconstruct, loop-filter,
 * update references.  Frames of one stream must be submitted in order.  Asynchronous. */
aa_status aa_decode_batch( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index );
/* Convenience = parse + upload + decode_batch(n=1): Decoder::get_frame_output (decoder.cc:125-135). */
aa_status aa_stream_decode( aa_stream * s, const uint8_t * data, size_t size, int * frame_index, int * shown );

/* ---- Device-side entropy decode (reference HOT LOOP #1: Frame::parse_macroblock_headers / parse_tokens,
 * frame.cc:95-137, tokens.cc:50-135, over BoolDecoder bool_decoder.hh:45-120).
 * aa_stream_parse runs the serial BoolDecoder on ONE host core per stream; a GPU consumes the output of ~1000 such cores.
 * aa_submit_frames instead does only the frame-header pre-pass on the host (decoder_state.hh:72-167: the part that is serial
 * across the frames of a stream) and hands the compressed frames themselves to the GPU, where every (stream, frame) is an
 * independent lane: macroblock headers and tokens are parsed in HBM, into the same records aa_stream_parse would have
 * produced.  Frames may be many per stream (in order) and of many streams; streams are processed in parallel by `threads`
 * host workers (0: one per core).  Asynchronous; aa_decode_batch of those frames orders itself behind the parse.
 * frame_index_out[i] (may be NULL) = index of frame i in its stream, -1 if it was not appended.  On a bitstream error the
 * failing frame and the later frames of ITS stream in this call are not appended, everything else is; the first error is
 * returned (same classes as aa_stream_parse). */
typedef struct aa_frame_in { aa_stream * stream; const uint8_t * data; size_t size; } aa_frame_in;
aa_status aa_submit_frames( aa_ctx * ctx, const aa_frame_in * frames, int n, int * frame_index_out, int threads );
/* Two-phase form, for callers that pipeline many batches and are bound by HBM: with AA_SUBMIT_DEFER_TOKENS the call does the
 * header pre-pass, the upload and the macroblock-header kernel (first partition) and allocates only the macroblock records;
 * the token kernel (DCT partitions) and the coefficient blocks -- 9/10 of a frame's records, worst-case sized -- wait for
 * aa_launch_tokens, which takes the oldest `max_batches` deferred batches (<= 0: all).  Anything that needs a deferred
 * frame's records (aa_decode_batch, aa_stream_frame_header, aa_stream_read_records) launches its batch's tokens itself. */
#define AA_SUBMIT_DEFER_TOKENS 1u
/* Routing.  By default a call whose streams are fewer than the host workers it may use (and at most 24) is parsed on the HOST --
 * one worker per stream, Parser::parse, records uploaded: the same records, sooner, because a frame on a GPU lane is a chain of
 * seconds and one core is worth ~75 lanes (an 8-chunk bundle: 4x the rate of the GPU parser) -- and everything larger on the GPU.
 * AA_SUBMIT_DEVICE / AA_SUBMIT_HOST force one or the other (so does the environment variable ALFALFA_AMD_ROUTE=device|host).
 * AA_SUBMIT_HOST on a call with MORE streams than that (frames that are needed at once: the key frames of the groups of pictures a
 * pipeline starts with -- 35 ms on a core, 2 s as a chain on a GPU lane) hands the frames to the context's HOST LANES: they take the
 * device route's header pre-pass and arena (frame indices at once; later frames of the same streams can be submitted immediately, on
 * any route), worker threads of the context -- as many as aa_host_cpus() -- parse macroblock headers and tokens the way a GPU lane
 * does and finish each frame with the same completion word.  THE CALL DOES NOT WAIT FOR THEM; aa_decode_batch,
 * aa_stream_frame_header, aa_stream_read_records and the release calls do, frame by frame.  Frames of a stream that uses
 * segmentation (its persistent map lives on the device) take the GPU's lanes all the same. */
#define AA_SUBMIT_DEVICE 2u
#define AA_SUBMIT_HOST 4u
aa_status aa_submit_frames_ex( aa_ctx * ctx, const aa_frame_in * frames, int n, int * frame_index_out, int threads, unsigned flags );
aa_status aa_launch_tokens( aa_ctx * ctx, int max_batches, int * launched_out );
/* Header of an appended frame.  For device-parsed frames the counts (num_coeff_blocks, num_intra_mbs, has_intra_mb) are known
 * only once the parse has run: this call waits for it. */
aa_status aa_stream_frame_header( aa_stream * s, int frame_index, aa_frame_header * out );
/* Test / debug view: a frame's parsed records as they sit in HBM (host- or device-parsed), copied back.  mb_out:
 * mb_width*mb_height records; coeff_out: up to coeff_capacity_blocks blocks of 16 (either may be NULL). */
aa_status aa_stream_read_records( aa_stream * s, int frame_index, aa_mb_info * mb_out, int16_t * coeff_out, size_t coeff_capacity_blocks );

/* Decoder::set_error_concealment for a stream decoder: applies to aa_stream_parse / aa_stream_decode AND to aa_submit_frames (the
 * frame tag is read by the host pre-pass; the GPU lanes read zeros past the end of what a frame has, like the host's). */
aa_status aa_stream_set_error_concealment( aa_stream * s, int on );
int aa_stream_error_concealment( const aa_stream * s );

/* Number of frames appended so far.  aa_stream_release_before: the caller is done with frames < first_kept -- their raster
 * handles are dropped (a raster lives on while a reference points at it: RasterHandle semantics, raster_handle.cc:113-122)
 * and the parsed records of the decoded ones go back to the context's pools (reused once queued kernels have run). */
int aa_stream_frame_count( const aa_stream * s );
aa_status aa_stream_release_before( aa_stream * s, int first_kept );
/* Forget all frames but keep decoder state? No: rewind the DEVICE half to frame 0 so the same resident
 * records can be decoded again (used by bench.py's steps; parser state is untouched). */
aa_status aa_stream_rewind( aa_stream * s );
/* Same, to frame `frame_index` (a key frame, or a frame whose reference rasters are all still held). */
aa_status aa_stream_rewind_to( aa_stream * s, int frame_index );

/* Output raster of a decoded frame (VP8Raster: three padded planes, stride = padded width, raster.hh:54-56).
 * Synchronises with the compute stream, then D2H.  Any pointer may be NULL. */
aa_status aa_stream_download( aa_stream * s, int frame_index, uint8_t * y, uint8_t * u, uint8_t * v );
/* The same without stalling the decoder (what a player that shows frames while decoding the next ones wants, player.cc:134-144):
 * the copy is queued on the context's COPY stream behind the work the compute stream holds at the time of the call and the
 * call returns; the planes -- pinned memory, aa_pinned_alloc -- are valid after aa_stream_download_wait (or aa_ctx_sync). */
aa_status aa_pinned_alloc( aa_ctx * ctx, size_t bytes, void ** out );
void aa_pinned_free( void * p );
aa_status aa_stream_download_async( aa_stream * s, int frame_index, uint8_t * y, uint8_t * u, uint8_t * v );
aa_status aa_stream_download_wait( aa_stream * s );
/* A whole batch at once -- what frontend/vp8decode.cc:78-93 / decode-bundle.cc:92-99 do with every shown frame, for n decoders in
 * lock step: frame frame_index[i] of streams[i] -> dst + i * stride (pinned memory, aa_pinned_alloc; stride a multiple of 16 and at
 * least a raster: Y, U, V planes back to back as VP8Raster pads them).  One gather kernel behind the reconstruction on the
 * compute stream and ONE copy on the copy stream, instead of 3 n plane copies; valid after aa_ctx_download_wait / aa_ctx_sync. */
aa_status aa_download_batch_async( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index, uint8_t * dst, size_t stride );
aa_status aa_ctx_download_wait( aa_ctx * ctx );
/* ... or only until at most max_in_flight of the batches queued by aa_download_batch_async are still on their way (oldest first): a
 * player that writes into a ring of r destination buffers calls this with r - 1 before it reuses one -- it waits for the copy that used
 * the buffer, not for the one queued a moment ago (what vp8decode.cc's display loop gets from double-buffered rasters). */
aa_status aa_ctx_download_wait_until( aa_ctx * ctx, int max_in_flight );
/* Device pointers of a frame's planes (valid while the frame's raster is alive). */
aa_status aa_stream_raster_device( aa_stream * s, int frame_index, void ** y, void ** u, void ** v );
/* Decoded frames to RGB on the device (what the reference's display shader does with every shown raster, display.cc): frame
 * frame_index[i] of streams[i] -> targets[i], the display rectangle (height rows of width pixels), all n in ONE kernel on the
 * compute stream behind the decode of those frames.  SMPTE 170M (BT.601) limited range; chroma co-sited horizontally, centred
 * vertically, bilinear with clamp-to-edge; exact integer definition in INTEGRATION.md.
 *   AA_RGB_U8_HWC3 / AA_RGB_U8_HWC4: rows of packed R G B (A = 255) bytes;  AA_RGB_*_CHW: three planes R, G, B of height rows
 *   targets[i].dst = first byte of row 0 (of plane R); row_stride >= width * bytes per pixel; plane_stride (CHW only) >= height *
 *   row_stride; nothing outside [row start, row start + width * bytes per pixel) of a row is written
 *   mean / std (float formats only; NULL = 0 / 1): out = (rgb / 255 - mean[c]) / std[c], computed in double, rounded to float and
 *   then to the output type (round to nearest even)
 * consumer_stream (a hipStream_t): the compute stream waits for it before the kernel (dst may have just been allocated there), and it
 * waits for the kernel.  NULL: no consumer stream, dst is valid after aa_ctx_sync (a consumer on HIP's null stream makes the two
 * waits itself, with events on aa_ctx_compute_stream). */
enum { AA_RGB_U8_HWC3 = 0, AA_RGB_U8_HWC4 = 1, AA_RGB_U8_CHW = 2, AA_RGB_F16_CHW = 3, AA_RGB_BF16_CHW = 4, AA_RGB_F32_CHW = 5 };
typedef struct aa_rgb_target { void * dst; int64_t row_stride; int64_t plane_stride; } aa_rgb_target;  /* bytes; plane_stride: CHW only */
aa_status aa_render_rgb_async( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index, int format,
                               const aa_rgb_target * targets, const double mean[3], const double std[3], void * consumer_stream );
/* Decoded frames scored against originals on the device (BaseRaster::quality, util/raster.cc:63-66 -> util/ssim.cc:57-71: x264's SSIM;
 * what Encoder::apply_best_loopfilter_settings, encode_with_minimum_ssim and xc-ssim ask of a raster): frame frame_index[i] of
 * streams[i] against originals[i], plane by plane over the PADDED planes (aa_raster_geometry for Y, half of it each way for U and V),
 * all n in one pair of kernels on the compute stream behind the decode of those frames.  Frames of different sizes may share a call.
 *   originals[i]: DEVICE pointers, row strides in bytes >= the plane's width; u, v are ignored for AA_QUALITY_Y.  The other side may be
 *   a decoded frame too: what aa_stream_raster_device returns, with strides = the padded widths.
 *   ssim_dev[i * planes + p] (device): the value aa_ssim_host returns for those two planes, bit for bit.
 *   sse_dev[i * planes + p] (device; NULL: not wanted): the exact sum of squared differences over the padded plane.
 * Nothing is copied to the host.  consumer_stream as for aa_render_rgb_async: the compute stream waits for it before the kernels and
 * it waits for them; NULL: the results are valid after aa_ctx_sync.  The frames must have been submitted and not released; one released
 * right after the call is still scored correctly.  No decoder state, hash or raster changes. */
enum { AA_QUALITY_Y = 1, AA_QUALITY_YUV = 3 };                       /* number of planes scored */
typedef struct aa_quality_ref { const void * y, * u, * v; int64_t y_stride, uv_stride; } aa_quality_ref;  /* DEVICE memory, bytes */
aa_status aa_quality_batch_async( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index,
                                  const aa_quality_ref * originals, int planes,
                                  double * ssim_dev, uint64_t * sse_dev, void * consumer_stream );
/* References::last/golden/alternative after the most recently SUBMITTED frame: frame indices (-1 = initial blank). */
aa_status aa_stream_references( const aa_stream * s, int * last, int * golden, int * alternate );
/* Identity of the three reference rasters as they stand now (all frames handed to aa_decode_batch so far applied): equal
 * numbers = the same raster; a number stays the same for as long as that raster is a reference.  Lets a binding keep ONE
 * handle per raster across frames, also for rasters no frame produced (the blank initial one, imported ones). */
aa_status aa_stream_reference_slots( const aa_stream * s, int slots[3] );
/* Replace all three references by a raster given as device planes (e.g. received by an RCCL broadcast over xGMI):
 * the entry-state hand-off of xc-decode-bundle (decoder.cc:171-175, References(EncoderStateDeserializer&)). */
aa_status aa_stream_import_reference( aa_stream * s, const void * y_dev, const void * u_dev, const void * v_dev );
/* Same from host planes. */
aa_status aa_stream_import_reference_host( aa_stream * s, const uint8_t * y, const uint8_t * u, const uint8_t * v );

/* Copy a decoded frame's raster into caller-owned DEVICE planes (e.g. a torch tensor used as RCCL send buffer);
 * asynchronous on the compute stream. */
aa_status aa_stream_export_raster( aa_stream * s, int frame_index, void * y_dev, void * u_dev, void * v_dev );
/* The stream's DecoderState (its parser), same blob as aa_parser_export_state / aa_parser_import_state. */
size_t aa_stream_state_size( const aa_stream * s );
aa_status aa_stream_export_state( const aa_stream * s, uint8_t * buf, size_t capacity );
aa_status aa_stream_import_state( aa_stream * s, const uint8_t * buf, size_t size );

/* The whole decoder as the reference writes it to a `.state` file: Decoder::serialize / Decoder::deserialize
 * (decoder.cc:54-81) = DecoderState + References (the LAST raster only; golden and alternative alias it after loading,
 * decoder.cc:171-197).  Files written by the reference's xc-enc -O / read by vp8decode -s and xc-decode-bundle load here
 * and vice versa.  Everything parsed must have been submitted; serialize waits for the device.  buf == NULL: size query. */
aa_status aa_stream_serialize( aa_stream * s, uint8_t * buf, size_t capacity, size_t * size );
aa_status aa_stream_deserialize( aa_stream * s, const uint8_t * buf, size_t size );

/* Hashes as the reference computes them (boost::hash_combine / hash_range, the pre-1.81 formula, over 64-bit size_t):
 *   DecoderState::hash (decoder.cc:266-281), BaseRaster::raw_hash of a decoded frame (raster.cc:52-61; computed on the host
 *   from a copy of the planes -- the recurrence is serial -- and cached per raster like HashCachedRaster),
 *   DecoderHash = {state, last, golden, alternative} and its hash (decoder.cc:143-153,482-490),
 *   Decoder::minihash = low 32 bits (decoder.cc:516-529): what xc-decode-bundle checks against IVF header bytes 28-31. */
aa_status aa_parser_state_hash( const aa_parser * p, uint64_t * out );
aa_status aa_stream_state_hash( aa_stream * s, uint64_t * out );
aa_status aa_stream_raster_hash( aa_stream * s, int frame_index, uint64_t * out );
aa_status aa_stream_decoder_hash( aa_stream * s, uint64_t parts[4], uint64_t * whole );
aa_status aa_stream_minihash( aa_stream * s, uint32_t * out );
/* The same hashes for MANY rasters / decoders in one call, without a download: every raster whose hash is not cached yet is one chain
 * of ONE kernel (k_hash_chains: a lane per chain -- the recurrence cannot be split, but chains are independent), on a stream of the
 * context's own that waits for what the compute stream holds at the call; rasters are deduplicated by device pointer (golden is
 * often the raster last is; fresh decoders share the context's blank raster).  The segment map of a decoder with segmentation on is
 * a chain too, of every call (maps change with every frame and have no cache); probability tables and adjustments are hashed on the
 * host in the call.  A lone 1080p chain takes tens of
 * milliseconds -- longer than the per-stream route -- and 1 440 of them take as long as one: for a handful of rasters use the
 * per-stream calls, for a chunk boundary of hundreds of decoders these.
 *   aa_hash_rasters_async   out[i] = aa_stream_raster_hash( streams[i], frame_index[i] ); same preconditions and errors.
 *   aa_hash_decoders_async  parts[4 i ..] / whole[i] / minihash[i] = aa_stream_decoder_hash / aa_stream_minihash of streams[i]
 *                           (any of the three may be NULL); everything parsed must have been submitted.
 *   aa_ctx_hash_wait        every outstanding call: the host arrays are written (they must live until then), and the per-raster
 *                           caches filled, so that the per-stream calls above answer without a download.  Waits for the hash stream,
 *                           not for the compute stream.  aa_ctx_sync does NOT commit hash calls.
 *   aa_ctx_hash_stats       out[0..3] = chains launched, bytes walked, rasters answered from the cache, cache entries filled.
 *   aa_ctx_hash_stream      the hipStream_t the kernels run on (for timing with events).
 * Every raster of a call is held from the call to the wait: a frame released right after the call is still hashed correctly and its
 * raster goes back to the pool at the wait.  At most 16 calls are outstanding; a seventeenth first commits the oldest.
 * aa_ctx_destroy and aa_stream_destroy commit outstanding calls first. */
aa_status aa_hash_rasters_async( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index, uint64_t * out );
aa_status aa_hash_decoders_async( aa_ctx * ctx, aa_stream * const * streams, int n, uint64_t * parts, uint64_t * whole, uint32_t * minihash );
aa_status aa_ctx_hash_wait( aa_ctx * ctx );
aa_status aa_ctx_hash_stats( aa_ctx * ctx, uint64_t out[4], int reset );
void * aa_ctx_hash_stream( aa_ctx * ctx );
/* Give back ONE frame: its raster handle (the raster lives on while a reference points at it) and, once decoded, its
 * parsed records -- what the destructor of the last RasterHandle of a frame does in the reference (raster_handle.cc:113-122). */
aa_status aa_stream_release_frame( aa_stream * s, int frame_index );
/* References{ last, golden, alternative } (Decoder( DecoderState, References ), decoder.cc:43-46): planes[i] = Y, U, V of
 * reference i, in HBM (is_host[i] == 0) or in host memory; references given by the same Y pointer become one raster.
 * aa_stream_reference_device / _download: the current References of a stream (which: 0 last, 1 golden, 2 alternative),
 * also before any frame (the blank raster) or after an import. */
aa_status aa_stream_set_references( aa_stream * s, const void * const planes[3][3], const int is_host[3] );
aa_status aa_stream_reference_device( aa_stream * s, int which, void ** y, void ** u, void ** v );
aa_status aa_stream_reference_download( aa_stream * s, int which, uint8_t * y, uint8_t * u, uint8_t * v );

/* Padded plane geometry for a display size (VP8Raster ctor, prediction.cc:94-97). */
void aa_raster_geometry( uint16_t width, uint16_t height, uint32_t * padded_width, uint32_t * padded_height );

/* Encoder feedback.  The reference update of Encoder::write_frame (encoder.cc:146-170: frame.decode +
 * frame.loopfilter + copy_to) IS aa_stream_decode of the frame it has just serialised.  What the encoder does BEFORE it knows
 * the loop-filter level -- Encoder::apply_best_loopfilter_settings (encoder.cc:459-516): filter a copy of the reconstruction
 * with every candidate level, score it against the original, keep the best -- is this call: `data` = the frame serialised
 * with any provisional level, `original_luma` = the original's padded luma plane (padded width x padded height, stride =
 * padded width: BaseRaster::Y(), util/raster.hh:54-60), candidates level_lo..level_hi (0..63; the reference tries 0..63 on
 * the first frame and last-1..last+1 afterwards, encoder.cc:477-487).  The stream's own state and references are not touched.
 * -> best_level / best_ssim by the reference's rule (ascending levels, stop at the first that does not improve);
 * ssim_out[level_hi - level_lo + 1] (optional): every candidate's score; rasters_out (optional, host): every candidate's
 * filtered raster, Y U V planes back to back. */
aa_status aa_stream_lf_search( aa_stream * s, const uint8_t * data, size_t size, const uint8_t * original_luma,
                               int level_lo, int level_hi, int * best_level, double * best_ssim, double * ssim_out, uint8_t * rasters_out );

/* The REBASE (Encoder::update_residues, reencode.cc:131-303, what xc-enc -r does with every inter frame of a chunk): the
 * prediction frame's modes and motion vectors are kept and its residues recomputed against the references the stream holds NOW, so
 * that the new frame decodes to the target picture from there -- predict, subtract from the target, forward DCT (WHT of the luma DCs
 * where a Y2 block is coded), plain division by the new header's factors, reconstruct (intra macroblocks predict from the new
 * frame's own unfiltered reconstruction).  One job = one (stream, new frame); jobs are independent and run as one pair of kernels on
 * the compute stream.  The call is synchronous: it returns with the records in the caller's arrays -- what aa_parser_parse would make
 * of the serialised frame (the choice of the token probabilities stays with the caller; Frame::serialize is aa_serialize_batch) -- and the
 * frame appended to its stream as aa_stream_append_records appends it: decode it with aa_decode_batch like any other frame (the stream's DecoderState is not advanced).
 * Errors (AA_ERR_ARGUMENT unless noted; nothing is appended to any stream of the call): key_frame set; segmentation_enabled
 * (AA_ERR_UNSUPPORTED: the reference quantises with the frame quantiser whatever the segment); null pointers; a header of another size;
 * a stream listed twice; a stream with a frame appended but not decoded (AA_ERR_LOGIC); coeff_capacity_blocks too small (the message
 * names the count needed; 25 per macroblock always suffice). */
typedef struct aa_rebase_job {
  aa_stream * stream;          /* predicted from ITS references; the new frame is appended to it */
  const aa_frame_header * hdr; /* header of the NEW frame: quant[0][*] are the factors used for division and reconstruction; loop filter
                                  fields, refresh / copy flags, sign bias as the caller wants them; key_frame must be 0 */
  const aa_mb_info * mbs;      /* prediction frame's records (aa_parser_parse / aa_stream_read_records): modes, ref_frame, vectors, b_modes,
                                  split_partition, segment_id, lf_level are taken; flags' residual bits, nz_mask, coeff_index are ignored */
  aa_quality_ref target;       /* DEVICE planes of the padded size, edge-extended by the caller */
  aa_mb_info * mbs_out; int16_t * coeffs_out; size_t coeff_capacity_blocks;   /* host */
  uint32_t num_coeff_blocks; int frame_index;                                  /* out */
} aa_rebase_job;
aa_status aa_rebase_batch( aa_ctx * ctx, aa_rebase_job * jobs, int n );
/* Where the last successful aa_rebase_batch of the context spent its time, in ms: out[0] the whole call (wall clock); [1] job table up
 * and the two kernels, [2] coefficients and masks down (HIP events on the compute stream, summed over the call's slices); [3] the
 * records built on the host, [4] the frames appended (wall clock).  For tools/rebase_probe.py. */
aa_status aa_rebase_last_timing( aa_ctx * ctx, double out[5] );
/* The same rebase with the new frame's records KEPT ON THE DEVICE: the two kernels of aa_rebase_batch, then k_rebase_count and
 * k_rebase_compact, which turn the masks and dense slots into the frame's records -- flags, nz_mask, coeff_index, the stored blocks in
 * parse order: byte for byte what aa_rebase_batch returns -- inside a piece of HBM that is the frame's from then on.  Nothing of the
 * records crosses the bus: per frame a few count words come down (the blocks stored per run of 256 macroblocks).  The frame is
 * appended to its stream and taken by aa_decode_batch, aa_serialize_batch, aa_stream_read_records, aa_stream_frame_header, release and
 * rewind like any other; a caller who wants the records on the host reads them back (aa_stream_read_records).  Synchronous.
 * num_coeff_blocks, num_intra_mbs (out): what the appended frame's header says.  Arguments, refusals and slicing as aa_rebase_batch's
 * (the messages begin "aa_rebase_device_batch:"; nothing is appended to any stream of a refused or failed call).
 * aa_rebase_last_timing reports this call too: [1] both uploads and the four kernels, [2] the count words down, [3] 0, [4] the
 * bookkeeping of the append.  (Still AA_ABI_VERSION 4: an addition, as the serialisation was.) */
typedef struct aa_rebase_device_job {
  aa_stream * stream; const aa_frame_header * hdr; const aa_mb_info * mbs; aa_quality_ref target;   /* as aa_rebase_job's */
  uint32_t num_coeff_blocks, num_intra_mbs; int frame_index;                                        /* out */
} aa_rebase_device_job;
aa_status aa_rebase_device_batch( aa_ctx * ctx, aa_rebase_device_job * jobs, int n );

/* The RE-ENCODE (Encoder::reencode_as_interframe, reencode.cc:38-129, the first thing xc-enc -r does to a chunk): the chunk's key frame
 * is encoded again as an inter frame predicted from the references the stream holds NOW -- the frame that joins two chunks.  Per
 * macroblock, in the reference's order and with its tie-breaks: the intra candidates (the B_PRED trial under AA_REENCODE_BEST, then
 * TM, H, V, DC), then ZEROMV, NEARESTMV, NEARMV and NEWMV from the last reference (NEWMV by the reference's diamond search; under
 * AA_REENCODE_REALTIME only where column % 4 == 0 and row % 4 == 0), the cheapest by its rate-distortion cost; then the chosen mode is
 * applied as the rebase applies it (forward DCT / WHT, plain division, reconstruction; an intra macroblock's uv_mode by distortion
 * alone).  One job = one (stream, new frame); jobs are independent, one workgroup each, one kernel on the compute stream.  The call
 * is synchronous: it returns with the records in the caller's arrays -- what aa_parser_parse would make of the serialised frame
 * (lf_level from hdr's level and the stream's current filter adjustments; segment_id 0; the choice of the token probabilities and the
 * loop-filter search stay with the caller; Frame::serialize is aa_serialize_batch) -- and, where `append` is set, the frame appended to its stream as aa_stream_append_records
 * appends it: decode it with aa_decode_batch.  With `append` clear nothing is appended and frame_index is -1: for a caller who runs
 * aa_stream_lf_search before the frame is final.  The vector costs come from the stream's current motion-vector probabilities.
 * Errors as aa_rebase_batch's (AA_ERR_ARGUMENT unless noted; nothing is appended to any stream of the call): key_frame set;
 * segmentation_enabled (AA_ERR_UNSUPPORTED, as the reference); null pointers; a header of another size; a stream listed twice; a stream
 * with a frame appended but not decoded (AA_ERR_LOGIC); coeff_capacity_blocks too small (the message names the count needed). */
#define AA_REENCODE_BEST 0
#define AA_REENCODE_REALTIME 1
typedef struct aa_reencode_job {
  aa_stream * stream;          /* predicted from ITS last reference; the new frame is appended to it */
  const aa_frame_header * hdr; /* header of the NEW frame, as aa_rebase_job's: quant[0][*], loop filter fields, refresh flags; key_frame must be 0 */
  aa_quality_ref target;       /* DEVICE planes of the padded size, edge-extended by the caller */
  int quality;                 /* AA_REENCODE_BEST / AA_REENCODE_REALTIME (xc-enc -q best / rt) */
  int append;                  /* != 0: append the frame to the stream */
  aa_mb_info * mbs_out; int16_t * coeffs_out; size_t coeff_capacity_blocks;   /* host */
  uint32_t num_coeff_blocks; int frame_index;                                  /* out */
} aa_reencode_job;
aa_status aa_reencode_batch( aa_ctx * ctx, aa_reencode_job * jobs, int n );
/* The same re-encode with the new frame's records KEPT ON THE DEVICE, as aa_rebase_device_batch keeps a rebased frame's: behind the
 * kernel of aa_reencode_batch, k_reencode_count and k_reencode_compact turn the records, masks and dense slots it left into the frame's
 * records -- flags, nz_mask, coeff_index, lf_level, the stored blocks in parse order: byte for byte what aa_reencode_batch returns --
 * inside a piece of HBM that is the frame's from then on.  Nothing of the records crosses the bus: per frame the blocks stored per run
 * of 256 macroblocks and the intra-row words come down (the modes are decided on the device, so the intra count and the diagonals are
 * derived from those words).  There is no `append` field: a frame that stays on the device is always appended to its stream, and is
 * taken by aa_decode_batch, aa_serialize_batch, aa_stream_read_records, aa_stream_frame_header, release and rewind like any other; a
 * caller who wants the records before the frame is final keeps using aa_reencode_batch with append = 0.  Synchronous.
 * num_coeff_blocks, num_intra_mbs (out): what the appended frame's header says.  Arguments, refusals and slicing as aa_reencode_batch's,
 * but for the coefficient capacity, which has no counterpart (the messages begin "aa_reencode_device_batch:"; nothing is appended to
 * any stream of a refused or failed call).  aa_reencode_last_timing reports this call too: [1] both uploads and the three kernels,
 * [2] the count words and row words down, [3] 0, [4] the bookkeeping of the append.  (Still AA_ABI_VERSION 4: an addition.) */
typedef struct aa_reencode_device_job {
  aa_stream * stream; const aa_frame_header * hdr; aa_quality_ref target; int quality;   /* as aa_reencode_job's */
  uint32_t num_coeff_blocks, num_intra_mbs; int frame_index;                              /* out */
} aa_reencode_device_job;
aa_status aa_reencode_device_batch( aa_ctx * ctx, aa_reencode_device_job * jobs, int n );
/* As aa_rebase_last_timing, for the last successful aa_reencode_batch (or aa_reencode_device_batch, see there): [1] job table and rate
 * models up and the kernel. */
aa_status aa_reencode_last_timing( aa_ctx * ctx, double out[5] );
/* How many macroblocks of an anti-diagonal a round of the re-encode kernel (and of the two kernels of the forward encoder) takes (1..16, default 16; also ALFALFA_AMD_REENC_SLOTS at
 * context creation): with a small cap the several-rounds-per-diagonal path runs on a small frame (tests). */
aa_status aa_ctx_set_reencode_slots( aa_ctx * ctx, int slots );

/* The FORWARD ENCODER (Encoder::encode_with_quantizer, encoder.cc:559-575: what xc-enc -i y4m -y QI -q best|rt does to every picture):
 * a raster in device memory becomes a new frame with the modes, vectors and coefficients the reference's single-pass encoder chooses --
 * a KEY frame (hdr->key_frame set; encode_raster<KeyFrame>, encode_intra.cc:388-456) or an INTER frame predicted from the stream's
 * current last reference (encode_raster<InterFrame>, encode_inter.cc:577-653).  One call may mix kinds, sizes and qualities; each kind is
 * one kernel over its jobs, a workgroup per job, on the re-encode's schedule (aa_ctx_set_reencode_slots caps its rounds too).
 * The jobs are aa_reencode_job / aa_reencode_device_job and mean what they mean there -- stream, header of the new frame (quant[0][*],
 * q_index, loop filter fields, refresh flags: the caller's; the probabilities are aa_serialize_batch's, optimise set), target planes on the
 * device, quality, append, the records out -- and the results are taken by aa_lf_search_decode_batch, aa_decode_batch and
 * aa_serialize_batch like a re-encoded frame's.  What differs from the re-encode:
 *   - the rate and distortion multipliers are update_rd_multipliers' (encoder.cc:178-193) of the job's quantiser, not 300 / 1;
 *   - a key frame weighs its 16x16 modes with the key frame's mode costs, tries B_PRED under both qualities, has no inter candidate and
 *     reads no reference: a key job needs no decoded frame, no reference and no prior state, and once it is appended and decoded all
 *     three references are the new frame (its lf_level is hdr's level, unadjusted: a key frame resets the stream's adjustments);
 *   - an inter frame's diamond search adds the rate of a site's vector to its SAD (sad_motion_vector_cost, costs.cc:231-240).
 * First pass only: plain division, no trellis.  Errors as aa_reencode_batch's (messages begin "aa_encode_batch: job i:" /
 * "aa_encode_device_batch: job i:"; nothing is appended to any stream of a refused call): null pointers; a quality that is none;
 * segmentation_enabled (AA_ERR_UNSUPPORTED, as the reference); a header of another size; a stream listed twice; an INTER job on a stream
 * whose last reference is no decoded frame (AA_ERR_LOGIC) or that holds a frame appended but not decoded (AA_ERR_LOGIC);
 * coeff_capacity_blocks too small.  (Still AA_ABI_VERSION 4: an addition.) */
typedef aa_reencode_job aa_encode_job;
typedef aa_reencode_device_job aa_encode_device_job;
aa_status aa_encode_batch( aa_ctx * ctx, aa_encode_job * jobs, int n );
aa_status aa_encode_device_batch( aa_ctx * ctx, aa_encode_device_job * jobs, int n );
/* The forward encoder WITH THE REFERENCE'S SECOND PASS for key frames (xc-enc --two-pass; encode_raster<KeyFrame> with two_pass_encoder_,
 * encode_intra.cc:409-439): the two calls above with, per job, a flag.  A KEY job whose flag is set runs, behind the first pass
 * (k_encode_key, unchanged), the decision a second time with every quantisation replaced by Encoder::trellis_quantize and
 * check_reset_y2 in front of the Y2 block's (k_encode_key2); its records, coefficients and reconstruction are the second pass's.  What
 * the first pass leaves behind reaches into the second as in the reference: the type its Y blocks ended with, the Y2 flag of a
 * macroblock that is B_PRED in the second pass, and the header's token_prob_update, which the reference never clears between the passes --
 * so the call also returns, per job, the FIRST pass's update table, for aa_serialize_batch to keep wherever the second pass makes no
 * update of its own (aa_serialize_job.first_pass_updates).  The feature is defined for a fresh encoder, as every stream xc-enc writes
 * has it: the first pass of this frame is the only history.  An inter job, and a key job whose flag is 0, take aa_encode_batch's path
 * untouched (the reference has no second pass for inter frames, encode_inter.cc:612-622); with every flag 0 the results are
 * aa_encode_batch's byte for byte.
 *   two_pass              [n]: job i's flag (ignored for an inter job)
 *   first_pass_updates    [n][AA_TWO_PASS_UPDATES], out: 1056 update flags then 1056 values ([4][8][3][11], zero where no flag) of job
 *                         i's first pass; all zero for a job that ran no second pass
 * Errors as aa_encode_batch's; null arrays are AA_ERR_ARGUMENT.  (Still AA_ABI_VERSION 4: an addition.) */
#define AA_TWO_PASS_UPDATES 2112
aa_status aa_encode_two_pass_batch( aa_ctx * ctx, aa_encode_job * jobs, int n, const uint8_t * two_pass, uint8_t * first_pass_updates );
aa_status aa_encode_two_pass_device_batch( aa_ctx * ctx, aa_encode_device_job * jobs, int n, const uint8_t * two_pass, uint8_t * first_pass_updates );
/* As aa_reencode_last_timing, for the last successful aa_encode_batch or aa_encode_device_batch (or their two-pass forms). */
aa_status aa_encode_last_timing( aa_ctx * ctx, double out[5] );

/* THE LOOP-FILTER LEVEL OF APPENDED FRAMES, searched for a whole batch (the last statement of Encoder::reencode_as_interframe,
 * reencode.cc:126: apply_best_loopfilter_settings, encoder.cc:459-516) -- and the DECODE of those frames.  Job i's frame is its stream's
 * next frame to decode, held as records: appended by aa_stream_append_records, aa_reencode_batch, aa_rebase_batch, or device-resident
 * (aa_reencode_device_batch, aa_rebase_device_batch), with whatever provisional level in its header.  All frames are reconstructed once,
 * unfiltered (aa_decode_batch's launches, the loop filter held back); then the jobs move together in rounds of K consecutive levels
 * (aa_ctx_set_lf_search_round; 4): k_lf_candidates copies every searching job's unfiltered raster to K candidate rasters and writes their
 * re-levelled records and job records, ONE loop-filter launch runs over all candidates, ONE scoring call over their luma planes, and
 * k_lf_choose continues the reference's rule per job -- levels in ascending order from level_lo, a candidate replaces the best only if its
 * score is greater, the first that does not ends the search -- so that one small copy per round tells the host who is done.  Level 0 is
 * scored on the unfiltered raster itself.  At the end the chosen level is set in every job's own records and job record, in place, and
 * the jobs' own rasters are filtered with it.
 *   measure   AA_LF_MEASURE_SSIM: x264's SSIM of the padded luma planes, the value aa_quality_batch_async / aa_ssim_host give;
 *             AA_LF_MEASURE_SSE: 1.0 - ( sse / ( double( pw ) * ph ) ) / ( 255.0 * 255.0 ) from the integer squared error of those planes.
 *   original  DEVICE; y and y_stride are read: the padded, edge-extended target luma (the re-encode's `target`).
 *   out       best_level; best_score, its score; evaluated, the candidates the rule consumed (the one that ended the search included).
 * After the call every job's stream stands where it would stand had the frame been appended with loop_filter_level = best_level,
 * filter_adjustments_enabled = 1 and zero mode / reference adjustments and then been handed to aa_decode_batch: the raster is the filtered
 * one, the references are updated, aa_stream_read_records gives lf_level = best_level's level of the record's segment (clamped to 0..63;
 * a device-resident frame is rewritten in its own piece of HBM, records the host holds too get the same), aa_stream_frame_header carries
 * the level, release and rewind treat the frame as a decoded one.  The stream's DecoderState is NOT touched: it is the header of the
 * written frame (aa_serialize_batch: lf_delta_update 1, every ref_lf_update / mode_lf_update 1 with delta 0) that zeroes the adjustments
 * for whoever parses the bytes.  The results do not depend on K or on how the jobs are sliced.  Synchronous.
 * Refusals (messages begin "aa_lf_search_decode_batch:"; a refused call decodes nothing, changes no stream and writes no output field):
 * AA_ERR_ARGUMENT for null pointers, n < 0, levels outside 0 <= lo <= hi <= 63, an unknown measure, a stream of another context or listed
 * twice, a key frame; AA_ERR_LOGIC for a frame that is not its stream's next to decode or whose records were released;
 * AA_ERR_UNSUPPORTED under AA_SCHEDULE_DIAGONAL (no row-pipelined loop filter to launch over the candidates).  n == 0 is AA_OK.
 * A call that FAILS behind its checks (AA_ERR_HIP, AA_ERR_NO_MEMORY: a launch, a copy, the pool, the watchdog; the message names this
 * call too) may have reconstructed the frames already: they then count as decoded -- next to decode is the frame behind them, the
 * references are updated -- with the UNFILTERED raster and the provisional level, and no output field is written.  Where the rasters
 * the frames predict from are still held, aa_stream_rewind_to( stream, frame_index ) and the same call again redo them.
 * Memory: the scratch of a slice is one piece; a piece of more than 128 MiB is given back to the device when its slice is over (it
 * does not stay parked in the context's pool), a smaller one is reused by the context's next compute-stream allocation of its size.
 * (Still AA_ABI_VERSION 4: an addition.) */
#define AA_LF_MEASURE_SSIM 0
#define AA_LF_MEASURE_SSE 1
typedef struct aa_lf_search_job {
  aa_stream * stream; int frame_index;
  aa_quality_ref original;
  int level_lo, level_hi;                          /* 0 <= lo <= hi <= 63 */
  int best_level, evaluated; double best_score;    /* out */
} aa_lf_search_job;
aa_status aa_lf_search_decode_batch( aa_ctx * ctx, aa_lf_search_job * jobs, int n, int measure );
/* Levels per job and round (1..8, default 4) and jobs per slice (0, the default: as many as an eighth of the memory limit, at most 8 GiB, holds -- the
 * scratch is jobs x levels x (raster + records + job record)): small numbers take small frames through several rounds and slices (tests). */
aa_status aa_ctx_set_lf_search_round( aa_ctx * ctx, int levels_per_round, int jobs_per_slice );
/* Where the last successful aa_lf_search_decode_batch spent its time, ms: out[0] the whole call (wall clock); HIP events on the compute
 * stream, summed over rounds and slices: [1] the unfiltered reconstruction, [2] round table up and k_lf_candidates, [3] the candidates'
 * loop filter, [4] the scoring, [5] k_lf_choose and the states down, [6] k_lf_finish and the final filter; [7] the number of rounds. */
aa_status aa_lf_search_last_timing( aa_ctx * ctx, double out[8] );

/* THE QUANTISER FOR A TARGET FRAME SIZE (Encoder::encode_with_target_size, encoder.cc:592-629: xc-enc -i y4m -F sizes, Salsify's rate
 * control) and the estimate it bisects over (Encoder::estimate_frame_size, size_estimation.cc: the number xc-enc -y prints as
 * [estimated size=N]).  An estimate is a complete first-pass encode of every FOURTH macroblock of the picture in each direction as a
 * frame of uint16( width / 4 ) x uint16( height / 4 ) pixels of its own -- macroblock (c, r) of it encodes the original's (4c, 4r),
 * searches and predicts at that position of the stream's last reference, takes its census, its clamp, its intra neighbours and the
 * real-time NEWMV rule from the small frame, and reconstructs at (c, r) -- serialised with one DCT partition, default token
 * probabilities' updates left out, prob_skip_false and the reference probabilities set as the reference sets them; the estimate is the
 * frame's size times 16.  k_estimate_key / k_estimate_inter make the decisions (the forward encoder's, on its schedule: a workgroup per
 * job, aa_ctx_set_reencode_slots caps its rounds), k_estimate_tokens counts the DCT partition's bytes on the device, the host writes
 * the first partition from the small frame's records.  Neither call appends a frame, advances a DecoderState or touches a reference.
 *   target     DEVICE planes of the padded size, edge-extended by the caller, as aa_encode_job's.
 *   key_frame  != 0: a key estimate (default probability tables, no reference, no carry); else the stream's current tables and last
 *              reference, as aa_encode_batch takes them.
 *   carry      in and out (an inter estimate; a key estimate leaves it alone).  [0..2]: prob_inter, prob_references_last,
 *              prob_references_golden of the reference's persistent estimate header -- optimize_interframe_probs replaces each only where
 *              its new value is above zero, so an estimate without an intra (or without an inter) macroblock is written with what the
 *              estimate BEFORE it left, across search steps and across frames; a new encoder starts from {0, 0, 0}.  [3] (in): 0 on the
 *              first inter frame behind a key frame, where the reference's vector cost tables are still all zero (the estimate does not fill
 *              them; the encode of an inter frame does), else 1: the stream's current motion-vector probabilities, as aa_encode_batch.
 * aa_target_size_batch moves all jobs together in rounds: one launch over every unfinished job, one candidate each -- the midpoint the
 * reference would try -- and the rule (qi_choose.hh) continued per job exactly as written there, `estimated_size <= target_size or
 * ( y_qi_min == y_qi_max and best_y_qi == 255 )` included; at most 7 rounds from the reference's ranges (aa_target_size_range), 8 from 0..127.  No extra candidate is evaluated: the carry makes the
 * visited sequence part of the result.  Out: q_index, the choice; estimates, their number; visited_q / visited_size, the candidates in
 * order with their estimates; carry, as the last estimate left it.
 * One pixel class is the library's own definition: the four pixels above and to the right of the last small-frame column's macroblocks
 * (rows >= 1) lie in the reference's full-size reconstruction raster beyond anything an estimate writes; here they are 0.
 * Both calls are synchronous.  Refusals (messages begin with the call's name; a refused call changes nothing and writes no output field):
 * AA_ERR_ARGUMENT for null pointers, n < 0, a stream of another context or listed twice, q_index / q_lo / q_hi outside 0..127,
 * q_lo > q_hi, a quality that is none, a row stride smaller than the padded plane's width; AA_ERR_LOGIC for an inter job whose stream's
 * last reference is not a decoded or imported raster, or whose stream holds a frame appended but not decoded; AA_ERR_UNSUPPORTED for a
 * display width or height under 4.  n == 0 is AA_OK.  (Still AA_ABI_VERSION 4: an addition.) */
typedef struct aa_estimate_size_job {
  aa_stream * stream;
  aa_quality_ref target;
  int key_frame, quality /* AA_REENCODE_BEST / AA_REENCODE_REALTIME */, q_index;
  uint8_t carry[4];            /* in, out */
  uint64_t size_out;           /* out */
} aa_estimate_size_job;
typedef struct aa_target_size_job {
  aa_stream * stream;
  aa_quality_ref target;
  int key_frame, quality, q_lo, q_hi;
  uint64_t target_size;
  uint8_t carry[4];            /* in, out */
  int q_index, estimates;      /* out */
  int visited_q[8]; uint64_t visited_size[8];   /* out: [0 .. estimates) */
} aa_target_size_job;
aa_status aa_estimate_size_batch( aa_ctx * ctx, aa_estimate_size_job * jobs, int n );
aa_status aa_target_size_batch( aa_ctx * ctx, aa_target_size_job * jobs, int n );
/* The range the reference's search starts from (encoder.cc:597-608): [4, 127], or last_q - 16 (where that is not below 4) .. last_q + 16
 * (capped at 127) around the index of the encoder's last frame, which it keeps under real-time quality only.  last_q < 0: none. */
void aa_target_size_range( int last_q, int * q_lo, int * q_hi );
/* Jobs per slice of a round (0, the default: as many as a slice of the rebase's scratch bound holds): 1 takes every job through a slice of
 * its own (tests). */
aa_status aa_ctx_set_target_size_round( aa_ctx * ctx, int jobs_per_slice );
/* Where the last successful aa_estimate_size_batch or aa_target_size_batch spent its time, ms: out[0] the whole call (wall clock); summed
 * over rounds and slices: [1] tables up and the decision kernels, [2] k_estimate_tokens, [3] results down (HIP events on the compute
 * stream), [4] the host's first partitions and the rule (wall clock); [5] the number of rounds. */
aa_status aa_target_size_last_timing( aa_ctx * ctx, double out[6] );

/* SERIALISATION (Frame::serialize, serializer.cc:388-829): frame `frame_index` of `stream`, held as records -- parsed from bytes, appended
 * by aa_rebase_batch / aa_reencode_batch / aa_stream_append_records, or device-resident (aa_rebase_device_batch, aa_reencode_device_batch: its 80-byte macroblock
 * records are copied back for the first partition, its blocks never leave HBM) -- becomes a VP8 frame in `out`.  The DCT partitions are written on the
 * device from the records where they lie, dense or packed (k_serialize_tokens: a lane per job and partition, partition p takes the
 * macroblock rows r % num_dct_partitions == p); meanwhile host workers, one job each, write the frame header and the macroblock headers of
 * the first partition from the macroblock records (the same boolean encoder, bool_writer.hh) and then put the frame together: tag, key-frame
 * start code and size, first partition, partition lengths, partitions.  What crosses the bus is the macroblock records (unless the host
 * still has them) and the compressed partitions.
 *   hdr           key_frame, show_frame, loop_filter_level, sharpness_level, num_dct_partitions, q_index, the refresh / copy / sign-bias flags,
 *                 segmentation_enabled and filter_adjustments_enabled (the header's Flagged<> bits) are written; mb_width / mb_height must be
 *                 the stream's.  num_dct_partitions need not be what the frame was parsed with.
 *   ext           the rest of the header, written as given (aa_parser_last_header_ext of a parse is a complete one).
 *   sub_modes     the sub-block modes of the SPLITMV macroblocks' partitions as aa_parser_last_sub_modes gives them for the frame the records
 *                 came from (for a rebased frame: its prediction frame, whose modes the rebase keeps), or NULL.  A listed mode is written where
 *                 it gives the record's vector; otherwise, and beyond the list, the first of LEFT4X4, ABOVE4X4, ZERO4X4 that gives the vector
 *                 is, else NEW4X4.  Every choice parses back to the same records; only the listed one is the original frame's bytes.
 *   probs_before  1101 bytes as aa_parser_get_probs returns them: the tables the frame's updates apply to (a key frame starts from the
 *                 defaults whatever they are); NULL: the stream's current tables.
 *   advance_state only with probs_before == NULL: afterwards the stream's DecoderState is advanced exactly as parsing the written frame
 *                 advances it (probabilities under refresh_entropy_probs, segmentation and its map, filter adjustments) -- a chain of frames is
 *                 then coded frame after frame against the state its predecessor left; hence a stream appears once per call.
 *   optimise      the reference's probability passes run on the device first (k_token_counts, k_token_probs) and overwrite the fields of
 *                 `ext` they decide: optimize_prob_skip (encoder.cc:442-457: skip_enabled 1, prob_skip_false), optimize_interframe_probs
 *                 (encode_inter.cc:525-575: prob_inter, prob_references_last, prob_references_golden, each only where calc_prob gives > 0;
 *                 inter frames) and optimize_probability_tables (encoder.cc:419-439: token_prob_update / token_prob, whatever the caller
 *                 put there), with calc_prob (encoder.cc:48-55) as written: 256 * false / total in integers, 0 when nothing was false,
 *                 an update where prob > 0 && prob != the table before the frame.  Counted are the Y, U and V blocks of EVERY macroblock
 *                 (Y2 blocks are not: serializer.cc:582-586).  On success `ext` holds the header as it was written.  Clear: as given.
 *   counts_out    optimise only, may be NULL: the counts the passes used, 2120 words: [4][8][3][11][2] {false, true}, then macroblocks with
 *                 coefficients, macroblocks by reference frame (intra, last, golden, altref), three zeros.  For tests.
 *   out, capacity host memory; size (out): the frame's bytes.  Nothing is written beyond capacity, on the host or in the device staging.
 * Records must be what a parse produces: nz_mask bit b set exactly when block b holds a coefficient the tokens code (a Y block beside a Y2
 * block from position 1 on), AA_MB_SKIP only with an empty nz_mask.  The call is synchronous.
 * Refusals (AA_ERR_ARGUMENT unless noted; nothing is written to any `out` and no state is advanced for any job of a refused call): null
 * pointers; a stream of another context or listed twice; frame_index out of range or released; num_dct_partitions not 1, 2, 4
 * or 8; advance_state together with probs_before; a header of another size, a key frame that holds inter macroblocks; a frame that does not fit its capacity (the message names the job and the bytes needed). */
typedef struct aa_serialize_job {
  aa_stream * stream; int frame_index;
  const aa_frame_header * hdr;
  aa_frame_header_ext * ext;
  int optimise, advance_state;
  const uint8_t * probs_before;
  const uint8_t * sub_modes; size_t num_sub_modes;
  uint8_t * out; size_t capacity;
  size_t size;                     /* out */
  uint32_t * counts_out;
} aa_serialize_job;
aa_status aa_serialize_batch( aa_ctx * ctx, aa_serialize_job * jobs, int n );
/* aa_serialize_batch for frames a two-pass encode made (aa_encode_two_pass_batch): first_pass_updates[n][AA_TWO_PASS_UPDATES] is what that
 * call returned per job.  A job with optimise keeps, wherever its own probability pass decides no update, the update the first pass made
 * (Encoder::optimize_probability_tables runs after each pass and never clears the header's token_prob_update, encoder.cc:419-439); a job
 * whose row is all zero, and a job without optimise, is aa_serialize_batch's.  (Still AA_ABI_VERSION 4: an addition.) */
aa_status aa_serialize_two_pass_batch( aa_ctx * ctx, aa_serialize_job * jobs, int n, const uint8_t * first_pass_updates );
/* Where the last successful aa_serialize_batch spent its time, ms: out[0] the whole call (wall clock); [1] job table up and k_serialize_tokens,
 * [2] partition sizes and partitions down (HIP events on the compute stream); [3] the host workers' frame headers and first partitions,
 * [4] assembly, the copy into `out` and the state advance (wall clock; [3] runs beside [1]).  For tools/serialize_probe.py. */
aa_status aa_serialize_last_timing( aa_ctx * ctx, double out[5] );
/* The same frame written by ONE host core from records in host memory (what aa_parser_parse / aa_stream_read_records / aa_rebase_batch
 * return: coeffs = dense blocks, a macroblock's at coeff_index): the host half's first partition and the token lanes' own statements
 * (serialize_common.hh) run on the host.  No device, no context; `optimise` is not offered here.  For tools/serialize_probe.py (the chain
 * on a host core beside the chain on a GPU lane) and for callers without a GPU at hand; it is no fallback of aa_serialize_batch, which
 * never calls it.  *size: the frame's bytes; more than capacity: AA_ERR_ARGUMENT, nothing written. */
aa_status aa_serialize_host( const aa_frame_header * hdr, const aa_frame_header_ext * ext, const uint8_t * probs_before, const aa_mb_info * mbs,
                             const int16_t * coeffs, const uint8_t * sub_modes, size_t num_sub_modes, uint8_t * out, size_t capacity, size_t * size );
/* aa_parser_last_header_ext for a stream's own parser: the frame aa_stream_parse / aa_stream_decode / aa_submit_frames parsed last. */
aa_status aa_stream_last_header_ext( const aa_stream * s, aa_frame_header_ext * out );
aa_status aa_stream_last_sub_modes( const aa_stream * s, uint8_t * out, size_t capacity, size_t * count );   /* (frames parsed by aa_stream_parse / aa_stream_decode) */

/* Quantizer::Quantizer( QuantIndices ) (quantization.cc:83-93): out = {y_dc, y_ac, y2_dc, y2_ac, uv_dc, uv_ac} for the base index
 * y_ac_qi and the header's deltas {y_dc, y2_dc, y2_ac, uv_dc, uv_ac} (NULL: all zero) -- aa_frame_header::quant[0] of a new frame. */
void aa_quant_factors( int y_ac_qi, const int8_t deltas[5], uint16_t out[6] );

/* BaseRaster::quality (util/raster.cc:63-66: x264's SSIM of two planes, stride = width) for planes in HOST memory. */
aa_status aa_ssim_host( const uint8_t * a, const uint8_t * b, int width, int height, double * out );

/* Per-kernel timing of the device half, measured with HIP events on the compute stream.
 * enable=1 brackets every kernel launch with events (serialises nothing beyond event records). */
typedef struct aa_kernel_stats {
  double recon_inter_ms, recon_intra_ms, loopfilter_ms;      /* summed launch durations */
  uint64_t recon_inter_launches, recon_intra_launches, loopfilter_launches;
  uint64_t macroblocks;                                      /* MBs processed by decode_batch calls */
  double parse_headers_ms, parse_tokens_ms;                  /* device-side entropy decode: k_parse_mb_headers, k_parse_tokens */
  uint64_t parse_launches;                                   /* aa_submit_frames calls timed */
  uint64_t parsed_macroblocks;                               /* MBs handed to the device parser */
  double recon_split_ms;                                     /* k_recon_inter on SPLITMV macroblocks (recon_inter_ms: k_recon_inter4 only) */
  uint64_t recon_split_launches;
  /* where the host stood still (always counted, profile on or off): waiting for released HBM pieces to come back because
   * hipMalloc was out of memory; waiting in aa_decode_batch for the device parser to finish the frames asked for */
  uint64_t pool_waits;
  double pool_wait_ms, parse_wait_ms;
  double bind_wait_ms;      /* aa_decode_batch waiting for one of its (16) raster-binding buffers: the compute stream is that far behind */
  double alloc_ms;          /* host time inside the device pool allocator (hipMalloc of new slabs included) */
  uint64_t slab_mallocs;    /* hipMalloc calls of the pool */
  /* token workers (device-side entropy decode) */
  uint64_t token_steps;     /* decode steps of the frames whose parse has been waited for (an upper bound on the bools decoded) */
  uint64_t token_frames;
  uint64_t worker_launches, worker_wgs;   /* worker grids launched / workgroups in them */
  uint64_t worker_retires;  /* grids told to finish so that their stream could take a new grid */
  uint64_t heap_grows;      /* pieces of memory mapped into the coefficient heap */
  uint64_t heap_mapped_bytes;
  uint64_t nomem_retries;   /* frames a lane handed back because the coefficient pool was empty, run again */
  uint64_t frames_evicted;  /* frames parsed ahead of their turn whose chunks were taken back for a frame needed now (parsed again later) */
  uint64_t host_routed_frames; /* frames of aa_submit_frames calls that were parsed by host cores (few streams: one worker per stream; else host lanes) */
  /* packed coefficient storage (aa_ctx_set_packed_coefficients) */
  /* (these two took the place of expand_ms / expand_launches: no expansion pass since round 6) */
  uint64_t row_handoff_stale_polls; /* ... of row_handoff_rereads: waits whose poll, repeated BEHIND the reads that saw the value, still returned the old one */
  uint64_t row_handoff_rereads;   /* waits of the row-pipelined kernels for the row above that the slow path's second look ended (kernels.hip, reread_progress):
                                     since the context was created, not reset; counts, not errors */
  uint64_t packed_frames, packed_words, packed_blocks;   /* frames stored packed, the 16-bit words they took, the dense blocks they stand for */
  /* host lanes: host_batch_parse_cpu_ms = the workers' summed parse time (CPU seconds x 1000; a diagnostic sum); host_batch_ms,
   * host_batch_parse_wall_ms, host_batch_arena_ms: 0 since round 5 (nothing of a submit call waits for host parsing any more) */
  double host_batch_ms, host_batch_parse_wall_ms, host_batch_parse_cpu_ms, host_batch_arena_ms;
  uint64_t pinned_allocs;
} aa_kernel_stats;
aa_status aa_ctx_profile( aa_ctx * ctx, int enable );
aa_status aa_ctx_kernel_stats( aa_ctx * ctx, aa_kernel_stats * out, int reset );

#ifdef __cplusplus
}
#endif
#endif /* ALFALFA_AMD_H */
