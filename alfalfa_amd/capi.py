"""ctypes binding of the C ABI (include/alfalfa_amd.h) -- the same stub a cgo/JNI/N-API binding would write.

The library is built in-tree by alfalfa_amd.build (hipcc, gfx950).  There is no Python or CPU
implementation behind these calls: if the library is missing or has no GPU to run on, they raise.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

AA_OK = 0
TWO_PASS_UPDATES = 2112      # AA_TWO_PASS_UPDATES: 1056 token_prob_update flags, then 1056 values
ERR_NAMES = {-1: "Invalid", -2: "Unsupported", -3: "LogicError", -4: "OutOfRange", -5: "HipError",
             -6: "NoDevice", -7: "BadArgument", -8: "NoMemory"}

AA_MB_HAS_NONZERO, AA_MB_HAS_Y2, AA_MB_INTER, AA_MB_SKIP, AA_MB_LF_SKIP_INNER = 1, 2, 4, 8, 16

MB_INFO_DTYPE = np.dtype([("y_mode", "u1"), ("uv_mode", "u1"), ("ref_frame", "u1"), ("segment_id", "u1"),
                          ("flags", "u1"), ("lf_level", "u1"), ("split_partition", "u1"), ("reserved", "u1"),
                          ("nz_mask", "<u4"), ("coeff_index", "<u4"), ("u", "u1", (64,))])
assert MB_INFO_DTYPE.itemsize == 80


class FrameHeader(C.Structure):
    _fields_ = [(n, C.c_uint8) for n in (
        "key_frame", "show_frame", "loop_filter_level", "sharpness_level", "num_dct_partitions",
        "segmentation_enabled", "filter_adjustments_enabled", "refresh_last", "refresh_golden",
        "refresh_alternate", "copy_buffer_to_golden", "copy_buffer_to_alternate", "sign_bias_golden",
        "sign_bias_alternate", "q_index", "has_intra_mb")] + [
        ("mb_width", C.c_uint16), ("mb_height", C.c_uint16), ("width", C.c_uint16), ("height", C.c_uint16),
        ("quant", (C.c_uint16 * 6) * 4), ("num_macroblocks", C.c_uint32), ("num_coeff_blocks", C.c_uint32),
        ("num_intra_mbs", C.c_uint32), ("compressed_size", C.c_uint32)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "quant"}
        d["quant"] = [[self.quant[s][k] for k in range(6)] for s in range(4)]
        return d


class FrameHeaderExt(C.Structure):
    """aa_frame_header_ext: what the bitstream's frame header holds beyond FrameHeader (bytes only; arrays as nested lists in dicts)."""
    _u8, _i8 = C.c_uint8, C.c_int8
    _fields_ = [(n, C.c_uint8) for n in ("color_space", "clamping_type", "filter_type", "refresh_entropy_probs", "update_mb_segmentation_map",
                                         "update_segment_feature_data", "segment_feature_mode", "lf_delta_update")] + [
        ("seg_quant_update", _u8 * 4), ("seg_quant", _i8 * 4), ("seg_lf_update", _u8 * 4), ("seg_lf", _i8 * 4),
        ("seg_tree_update", _u8 * 3), ("seg_tree_probs", _u8 * 3), ("skip_enabled", _u8), ("prob_skip_false", _u8),
        ("ref_lf_update", _u8 * 4), ("ref_lf_delta", _i8 * 4), ("mode_lf_update", _u8 * 4), ("mode_lf_delta", _i8 * 4),
        ("q_update", _u8 * 5), ("q_delta", _i8 * 5), ("prob_inter", _u8), ("prob_references_last", _u8), ("prob_references_golden", _u8),
        ("intra_16x16_update", _u8), ("intra_16x16_prob", _u8 * 4), ("intra_chroma_update", _u8), ("intra_chroma_prob", _u8 * 3),
        ("mv_prob_update", _u8 * 38), ("mv_prob", _u8 * 38), ("token_prob_update", _u8 * 1056), ("token_prob", _u8 * 1056)]

    def as_dict(self):
        """Scalars as ints, arrays as lists (mv_*: 38 = [2][19], token_*: 1056 = [4][8][3][11], flat)."""
        return {n: (getattr(self, n) if isinstance(getattr(self, n), int) else list(getattr(self, n))) for n, _ in self._fields_}

    @classmethod
    def from_dict(cls, d):
        x = cls()
        for n, t in cls._fields_:
            if n not in d:
                continue
            if hasattr(t, "_length_"):
                v = [int(e) for e in np.asarray(d[n]).reshape(-1)]
                if len(v) != t._length_:
                    raise ValueError("FrameHeaderExt: %s holds %d values, not %d" % (n, len(v), t._length_))
                setattr(x, n, t(*v))
            else:
                setattr(x, n, int(d[n]))
        return x


class SerializeJob(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("frame_index", C.c_int), ("hdr", C.POINTER(FrameHeader)), ("ext", C.POINTER(FrameHeaderExt)),
                ("optimise", C.c_int), ("advance_state", C.c_int), ("probs_before", C.c_void_p), ("sub_modes", C.c_void_p), ("num_sub_modes", C.c_size_t), ("out", C.c_void_p), ("capacity", C.c_size_t),
                ("size", C.c_size_t), ("counts_out", C.c_void_p)]


class FrameIn(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("data", C.c_char_p), ("size", C.c_size_t)]


class KernelStats(C.Structure):
    _fields_ = [("recon_inter_ms", C.c_double), ("recon_intra_ms", C.c_double), ("loopfilter_ms", C.c_double),
                ("recon_inter_launches", C.c_uint64), ("recon_intra_launches", C.c_uint64),
                ("loopfilter_launches", C.c_uint64), ("macroblocks", C.c_uint64),
                ("parse_headers_ms", C.c_double), ("parse_tokens_ms", C.c_double), ("parse_launches", C.c_uint64),
                ("parsed_macroblocks", C.c_uint64), ("recon_split_ms", C.c_double), ("recon_split_launches", C.c_uint64),
                ("pool_waits", C.c_uint64), ("pool_wait_ms", C.c_double), ("parse_wait_ms", C.c_double),
                ("bind_wait_ms", C.c_double), ("alloc_ms", C.c_double), ("slab_mallocs", C.c_uint64),
                ("token_steps", C.c_uint64), ("token_frames", C.c_uint64), ("worker_launches", C.c_uint64), ("worker_wgs", C.c_uint64),
                ("worker_retires", C.c_uint64), ("heap_grows", C.c_uint64), ("heap_mapped_bytes", C.c_uint64), ("nomem_retries", C.c_uint64), ("frames_evicted", C.c_uint64), ("host_routed_frames", C.c_uint64),
                ("row_handoff_stale_polls", C.c_uint64), ("row_handoff_rereads", C.c_uint64), ("packed_frames", C.c_uint64), ("packed_words", C.c_uint64), ("packed_blocks", C.c_uint64),
                ("host_batch_ms", C.c_double), ("host_batch_parse_wall_ms", C.c_double), ("host_batch_parse_cpu_ms", C.c_double), ("host_batch_arena_ms", C.c_double),
                ("pinned_allocs", C.c_uint64)]


class CtxInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("memory_limit_bytes", "pool_bytes", "pool_free_bytes", "pool_pending_bytes", "heap_mapped_bytes", "heap_limit_bytes", "heap_used_bytes",
                                          "pinned_host_bytes")] + [
        (n, C.c_uint32) for n in ("heap_is_virtual", "token_lanes_per_workgroup", "token_workgroups_capacity", "token_workgroups_alive",
                                  "token_lane_lds_bytes", "token_workgroup_lds_bytes", "jobs_waiting", "compute_units")] + [
        ("heap_free_chunks", C.c_int32), ("lanes_starved", C.c_uint32), ("token_profile", C.c_uint64 * 8),
        ("packed_coefficients", C.c_uint32), ("lane_per_partition", C.c_uint32), ("clock_mhz", C.c_uint32), ("host_share_ms", C.c_uint32), ("host_rate_kb_per_ms", C.c_uint32), ("reserved1", C.c_uint32), ("stream_concurrency", C.c_uint32), ("streams_needed", C.c_uint32),
        ("host_waited_parse_ms", C.c_uint32), ("host_waited_compute_ms", C.c_uint32)]


AA_RGB_U8_HWC3, AA_RGB_U8_HWC4, AA_RGB_U8_CHW, AA_RGB_F16_CHW, AA_RGB_BF16_CHW, AA_RGB_F32_CHW = range(6)


class RgbTarget(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("row_stride", C.c_int64), ("plane_stride", C.c_int64)]


AA_QUALITY_Y, AA_QUALITY_YUV = 1, 3


class QualityRef(C.Structure):
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_stride", C.c_int64), ("uv_stride", C.c_int64)]


class RebaseJob(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("hdr", C.POINTER(FrameHeader)), ("mbs", C.c_void_p), ("target", QualityRef),
                ("mbs_out", C.c_void_p), ("coeffs_out", C.c_void_p), ("coeff_capacity_blocks", C.c_size_t),
                ("num_coeff_blocks", C.c_uint32), ("frame_index", C.c_int)]


class RebaseDeviceJob(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("hdr", C.POINTER(FrameHeader)), ("mbs", C.c_void_p), ("target", QualityRef),
                ("num_coeff_blocks", C.c_uint32), ("num_intra_mbs", C.c_uint32), ("frame_index", C.c_int)]


class ReencodeJob(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("hdr", C.POINTER(FrameHeader)), ("target", QualityRef), ("quality", C.c_int), ("append", C.c_int),
                ("mbs_out", C.c_void_p), ("coeffs_out", C.c_void_p), ("coeff_capacity_blocks", C.c_size_t),
                ("num_coeff_blocks", C.c_uint32), ("frame_index", C.c_int)]


class ReencodeDeviceJob(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("hdr", C.POINTER(FrameHeader)), ("target", QualityRef), ("quality", C.c_int),
                ("num_coeff_blocks", C.c_uint32), ("num_intra_mbs", C.c_uint32), ("frame_index", C.c_int)]


EncodeJob, EncodeDeviceJob = ReencodeJob, ReencodeDeviceJob       # aa_encode_job / aa_encode_device_job are typedefs of them



class EstimateSizeJob(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("target", QualityRef), ("key_frame", C.c_int), ("quality", C.c_int), ("q_index", C.c_int), ("carry", C.c_uint8 * 4),
                ("size_out", C.c_uint64)]


class TargetSizeJob(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("target", QualityRef), ("key_frame", C.c_int), ("quality", C.c_int), ("q_lo", C.c_int), ("q_hi", C.c_int),
                ("target_size", C.c_uint64), ("carry", C.c_uint8 * 4), ("q_index", C.c_int), ("estimates", C.c_int), ("visited_q", C.c_int * 8),
                ("visited_size", C.c_uint64 * 8)]


AA_LF_MEASURE_SSIM, AA_LF_MEASURE_SSE = 0, 1


class LfSearchJob(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("frame_index", C.c_int), ("original", QualityRef), ("level_lo", C.c_int), ("level_hi", C.c_int),
                ("best_level", C.c_int), ("evaluated", C.c_int), ("best_score", C.c_double)]


class AlfalfaError(RuntimeError):
    """Mirrors the reference's exception types (exception.hh:76-98) by name in `.kind`."""

    def __init__(self, code, message):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, str(code)), message))
        self.code, self.kind, self.message = code, ERR_NAMES.get(code, str(code)), message


# every entry point declared in include/alfalfa_amd.h: (name, restype, argtypes)
_P = C.c_void_p
_U8P = C.POINTER(C.c_uint8)
SYMBOLS = [
    ("aa_last_error", C.c_char_p, []), ("aa_abi_version", C.c_int, []), ("aa_runtime_prepare", C.c_int, []), ("aa_host_cpus", C.c_int, []), ("aa_device_count", C.c_int, []),
    ("aa_parser_create", C.c_int, [C.c_uint16, C.c_uint16, C.POINTER(_P)]), ("aa_parser_destroy", None, [_P]),
    ("aa_parser_parse", C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(FrameHeader), _P, _P]),
    ("aa_parser_get_probs", C.c_int, [_P, _U8P]), ("aa_parser_set_error_concealment", C.c_int, [_P, C.c_int]),
    ("aa_parse_frame_tag", C.c_int, [C.c_char_p, C.c_size_t, C.c_uint16, C.c_uint16, C.c_int] + [C.POINTER(C.c_int)] * 4),
    ("aa_stream_set_error_concealment", C.c_int, [_P, C.c_int]), ("aa_stream_error_concealment", C.c_int, [_P]),
    ("aa_parser_get_segmentation", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int8), C.POINTER(C.c_int8), _U8P]),
    ("aa_parser_get_filter_adjustments", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int8), C.POINTER(C.c_int8)]),
    ("aa_parser_serialize_state", C.c_int, [_P, _P, C.c_size_t, _P]), ("aa_parser_deserialize_state", C.c_int, [_P, _P, C.c_size_t]),
    ("aa_stream_serialize", C.c_int, [_P, _P, C.c_size_t, _P]), ("aa_stream_deserialize", C.c_int, [_P, _P, C.c_size_t]),
    ("aa_parser_state_size", C.c_size_t, [_P]), ("aa_parser_export_state", C.c_int, [_P, _P, C.c_size_t]),
    ("aa_parser_import_state", C.c_int, [_P, C.c_char_p, C.c_size_t]),
    ("aa_stream_state_size", C.c_size_t, [_P]), ("aa_stream_export_state", C.c_int, [_P, _P, C.c_size_t]),
    ("aa_stream_import_state", C.c_int, [_P, C.c_char_p, C.c_size_t]),
    ("aa_stream_export_raster", C.c_int, [_P, C.c_int, _P, _P, _P]),
    ("aa_ctx_create", C.c_int, [C.c_int, C.POINTER(_P)]), ("aa_ctx_destroy", None, [_P]), ("aa_ctx_sync", C.c_int, [_P]),
    ("aa_ctx_memory", C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("aa_ctx_set_memory_limit", C.c_int, [_P, C.c_size_t]), ("aa_ctx_set_packed_coefficients", C.c_int, [_P, C.c_int]), ("aa_ctx_set_host_share_ms", C.c_int, [_P, C.c_double]), ("aa_ctx_set_lane_per_partition", C.c_int, [_P, C.c_int]), ("aa_ctx_get_info", C.c_int, [_P, C.POINTER(CtxInfo)]),
    ("aa_ctx_set_schedule", C.c_int, [_P, C.c_int]), ("aa_ctx_clear_error", C.c_int, [_P]), ("aa_ctx_compute_stream", _P, [_P]), ("aa_ctx_copy_stream", _P, [_P]),
    ("aa_stream_create", C.c_int, [_P, C.c_uint16, C.c_uint16, C.POINTER(_P)]), ("aa_stream_destroy", None, [_P]),
    ("aa_stream_parse", C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(FrameHeader)]),
    ("aa_stream_append_records", C.c_int, [_P, C.POINTER(FrameHeader), _P, _P, C.POINTER(C.c_int)]),
    ("aa_stream_upload", C.c_int, [_P]), ("aa_stream_release_staging", C.c_int, [_P]),
    ("aa_decode_batch", C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(C.c_int)]),
    ("aa_stream_decode", C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("aa_submit_frames", C.c_int, [_P, C.POINTER(FrameIn), C.c_int, C.POINTER(C.c_int), C.c_int]),
    ("aa_submit_frames_ex", C.c_int, [_P, C.POINTER(FrameIn), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_uint]),
    ("aa_launch_tokens", C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    ("aa_ssim_host", C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("aa_stream_lf_search", C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.c_void_p]),
    ("aa_stream_frame_header", C.c_int, [_P, C.c_int, C.POINTER(FrameHeader)]),
    ("aa_stream_read_records", C.c_int, [_P, C.c_int, _P, _P, C.c_size_t]),
    ("aa_stream_frame_count", C.c_int, [_P]), ("aa_stream_release_before", C.c_int, [_P, C.c_int]),
    ("aa_stream_rewind", C.c_int, [_P]), ("aa_stream_rewind_to", C.c_int, [_P, C.c_int]),
    ("aa_stream_download", C.c_int, [_P, C.c_int, _P, _P, _P]),
    ("aa_pinned_alloc", C.c_int, [_P, C.c_size_t, C.POINTER(_P)]), ("aa_pinned_free", None, [_P]),
    ("aa_stream_download_async", C.c_int, [_P, C.c_int, _P, _P, _P]), ("aa_stream_download_wait", C.c_int, [_P]),
    ("aa_download_batch_async", C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(C.c_int), _P, C.c_size_t]), ("aa_ctx_download_wait", C.c_int, [_P]), ("aa_ctx_download_wait_until", C.c_int, [_P, C.c_int]),
    ("aa_stream_raster_device", C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    ("aa_render_rgb_async", C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(RgbTarget),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    ("aa_quality_batch_async", C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(C.c_int), C.POINTER(QualityRef), C.c_int, _P, _P, _P]),
    ("aa_rebase_batch", C.c_int, [_P, C.POINTER(RebaseJob), C.c_int]),
    ("aa_rebase_device_batch", C.c_int, [_P, C.POINTER(RebaseDeviceJob), C.c_int]),
    ("aa_rebase_last_timing", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("aa_reencode_batch", C.c_int, [_P, C.POINTER(ReencodeJob), C.c_int]),
    ("aa_reencode_device_batch", C.c_int, [_P, C.POINTER(ReencodeDeviceJob), C.c_int]),
    ("aa_reencode_last_timing", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("aa_ctx_set_reencode_slots", C.c_int, [_P, C.c_int]),
    ("aa_encode_batch", C.c_int, [_P, C.POINTER(ReencodeJob), C.c_int]),
    ("aa_encode_device_batch", C.c_int, [_P, C.POINTER(ReencodeDeviceJob), C.c_int]),
    ("aa_encode_two_pass_batch", C.c_int, [_P, C.POINTER(ReencodeJob), C.c_int, _P, _P]),
    ("aa_encode_two_pass_device_batch", C.c_int, [_P, C.POINTER(ReencodeDeviceJob), C.c_int, _P, _P]),
    ("aa_serialize_two_pass_batch", C.c_int, [_P, C.POINTER(SerializeJob), C.c_int, _P]),
    ("aa_encode_last_timing", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("aa_estimate_size_batch", C.c_int, [_P, C.POINTER(EstimateSizeJob), C.c_int]), ("aa_target_size_batch", C.c_int, [_P, C.POINTER(TargetSizeJob), C.c_int]),
    ("aa_target_size_range", None, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]), ("aa_ctx_set_target_size_round", C.c_int, [_P, C.c_int]),
    ("aa_target_size_last_timing", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("aa_lf_search_decode_batch", C.c_int, [_P, C.POINTER(LfSearchJob), C.c_int, C.c_int]),
    ("aa_ctx_set_lf_search_round", C.c_int, [_P, C.c_int, C.c_int]), ("aa_lf_search_last_timing", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("aa_parser_last_header_ext", C.c_int, [_P, C.POINTER(FrameHeaderExt)]), ("aa_stream_last_header_ext", C.c_int, [_P, C.POINTER(FrameHeaderExt)]),
    ("aa_parser_last_sub_modes", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]), ("aa_stream_last_sub_modes", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("aa_serialize_host", C.c_int, [C.POINTER(FrameHeader), C.POINTER(FrameHeaderExt), _P, _P, _P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("aa_serialize_batch", C.c_int, [_P, C.POINTER(SerializeJob), C.c_int]), ("aa_serialize_last_timing", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("aa_quant_factors", None, [C.c_int, C.POINTER(C.c_int8), C.POINTER(C.c_uint16)]),
    ("aa_stream_references", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("aa_stream_reference_slots", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("aa_stream_import_reference", C.c_int, [_P, _P, _P, _P]),
    ("aa_stream_import_reference_host", C.c_int, [_P, _P, _P, _P]),
    ("aa_parser_state_hash", C.c_int, [_P, C.POINTER(C.c_uint64)]), ("aa_stream_state_hash", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("aa_stream_raster_hash", C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    ("aa_stream_decoder_hash", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("aa_stream_minihash", C.c_int, [_P, C.POINTER(C.c_uint32)]),
    ("aa_hash_rasters_async", C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    ("aa_hash_decoders_async", C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    ("aa_ctx_hash_wait", C.c_int, [_P]), ("aa_ctx_hash_stats", C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]), ("aa_ctx_hash_stream", _P, [_P]),
    ("aa_stream_release_frame", C.c_int, [_P, C.c_int]),
    ("aa_stream_set_references", C.c_int, [_P, C.POINTER(_P * 3), C.POINTER(C.c_int)]),
    ("aa_stream_reference_device", C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    ("aa_stream_reference_download", C.c_int, [_P, C.c_int, _P, _P, _P]),
    ("aa_raster_geometry", None, [C.c_uint16, C.c_uint16, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("aa_ctx_profile", C.c_int, [_P, C.c_int]), ("aa_ctx_kernel_stats", C.c_int, [_P, C.POINTER(KernelStats), C.c_int]),
]

_lib = None


def lib():
    """Load (building if stale) the native library.  Raises if it cannot be built or loaded: no fallback."""
    global _lib
    if _lib is None:
        path = _build.LIB
        if os.environ.get("ALFALFA_AMD_LIB"):              # (A/B runs of a differently built library; never set in production)
            path = os.environ["ALFALFA_AMD_LIB"]
        elif _build.stale():
            if os.path.exists(_build.HIPCC):
                _build.build()
            elif not os.path.exists(path):
                raise RuntimeError("libalfalfa_amd.so is missing and hipcc is not available: there is no CPU fallback")
        # One HIP runtime per process: torch's HIP libraries ask for libamdhip64.so / libhsa-runtime64.so by these bare names and
        # would start a second runtime of their own beside ours (whose loader names are versioned) -- one that then finds no GPU.
        # Loaded under these names first, they are the ones a torch imported later binds to (or torch's, if it came first).
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            try:
                C.CDLL(name, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
        L = C.CDLL(path)
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(L, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = restype, argtypes
        L.aa_runtime_prepare()             # GPU_MAX_HW_QUEUES=16 unless the environment says otherwise: before this process's first HIP call, if it is ours
        _lib = L
    return _lib


def check(rc):
    if rc != AA_OK:
        raise AlfalfaError(rc, lib().aa_last_error().decode("utf-8", "replace"))


def device_count():
    return lib().aa_device_count()


def quant_factors(qi, deltas=None):
    """Quantizer::Quantizer( QuantIndices ) (quantization.cc:83-93) -> [y_dc, y_ac, y2_dc, y2_ac, uv_dc, uv_ac] for the base index qi
    and the header's deltas (y_dc, y2_dc, y2_ac, uv_dc, uv_ac), None = all zero: a new frame header's quant[0] (aa_quant_factors)."""
    out = (C.c_uint16 * 6)()
    d = None
    if deltas is not None:
        if len(deltas) != 5:
            raise ValueError("quant_factors: deltas are (y_dc, y2_dc, y2_ac, uv_dc, uv_ac)")
        d = (C.c_int8 * 5)(*deltas)
    lib().aa_quant_factors(int(qi), d, out)
    return list(out)


def target_size_range(last_q=None):
    """The range Encoder::encode_with_target_size searches (encoder.cc:597-608) -> (q_lo, q_hi): (4, 127), or around the quantiser index
    of the encoder's last frame -- last_q - 16 where that is not below 4, last_q + 16 capped at 127.  The reference keeps a last index
    under real-time quality only: pass last_q there and nowhere else (aa_target_size_range)."""
    lo, hi = C.c_int(), C.c_int()
    lib().aa_target_size_range(-1 if last_q is None else int(last_q), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def estimate_carry():
    """The carry a stream's first inter estimate starts from (Context.estimate_frame_sizes, Context.target_size_q): the three reference
    probabilities of a default-constructed header, all zero, and vector cost tables that are not filled yet.  Byte 3 becomes 1 once the
    stream's first inter frame has been ENCODED; bytes 0..2 are handed on from every inter estimate to the next."""
    return (0, 0, 0, 0)


def raster_geometry(width, height):
    pw, ph = C.c_uint32(), C.c_uint32()
    lib().aa_raster_geometry(width, height, C.byref(pw), C.byref(ph))
    return pw.value, ph.value
