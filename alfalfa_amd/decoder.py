"""Python mirror of the reference's decoder surface for THIS path, over the C ABI.

Names follow the reference: Parser ~ DecoderState::parse_and_apply (decoder_state.hh:72-167),
Decoder ~ Decoder (decoder.hh:244-300: decode_frame / get_frame_output / parse_and_decode_frame /
get_references), FilePlayer ~ FilePlayer (player.hh:66-97: advance / eof), DecodeBatch = N
independent streams decoded in lockstep (ExCamera chunks / GOPs, one batch per GPU).
"""
import collections
import ctypes as C
import struct

import numpy as np

from . import capi
from .capi import AlfalfaError, FrameHeader, MB_INFO_DTYPE  # noqa: F401


Quality = collections.namedtuple("Quality", ["ssim", "sse"])


class Parser:
    """Host-only bitstream parser with the reference's persistent DecoderState."""

    def __init__(self, width, height):
        self.L = capi.lib()
        self.h = C.c_void_p()
        capi.check(self.L.aa_parser_create(width, height, C.byref(self.h)))
        self.width, self.height = width, height
        self.mbw, self.mbh = (width + 15) // 16, (height + 15) // 16
        n = self.mbw * self.mbh
        self._mb = np.zeros(n, dtype=MB_INFO_DTYPE)
        self._coeff = np.zeros(n * 25 * 16, dtype=np.int16)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.aa_parser_destroy(self.h); self.h = None

    def parse(self, frame_bytes):
        """-> (header dict, mb_info structured array [mbh, mbw], coefficient blocks [n, 16])."""
        hdr = FrameHeader()
        capi.check(self.L.aa_parser_parse(self.h, frame_bytes, len(frame_bytes), C.byref(hdr),
                                          self._mb.ctypes.data_as(C.c_void_p), self._coeff.ctypes.data_as(C.c_void_p)))
        h = hdr.as_dict()
        return h, self._mb.copy().reshape(self.mbh, self.mbw), self._coeff[:h["num_coeff_blocks"] * 16].copy().reshape(-1, 16)

    def header_ext(self):
        """The rest of the header of the frame parsed last (aa_parser_last_header_ext) -> dict of the fields of aa_frame_header_ext:
        with the header dict of parse() it is everything a serialiser writes (Context.serialize_frames)."""
        x = capi.FrameHeaderExt()
        capi.check(self.L.aa_parser_last_header_ext(self.h, C.byref(x)))
        return x.as_dict()

    def sub_modes(self):
        """The sub-block modes (10 LEFT4X4 .. 13 NEW4X4) of the SPLITMV partitions of the frame parsed last, in bitstream order
        (aa_parser_last_sub_modes) -> uint8 array: what the records do not hold and a byte-exact serialisation needs."""
        n = C.c_size_t()
        capi.check(self.L.aa_parser_last_sub_modes(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.uint8)
        capi.check(self.L.aa_parser_last_sub_modes(self.h, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)))
        return out[:n.value]

    def set_error_concealment(self, on):
        """Decoder::set_error_concealment (decoder.hh:298): accept frames that end early."""
        capi.check(self.L.aa_parser_set_error_concealment(self.h, int(on)))

    def export_state(self):
        """DecoderState as bytes (host half of the entry-state hand-off, decoder.cc:43-46)."""
        n = self.L.aa_parser_state_size(self.h)
        buf = (C.c_uint8 * n)()
        capi.check(self.L.aa_parser_export_state(self.h, buf, n))
        return bytes(buf)

    def import_state(self, blob):
        capi.check(self.L.aa_parser_import_state(self.h, blob, len(blob)))

    def serialize_state(self):
        """DecoderState in the reference's wire format (DecoderState::serialize, decoder.cc:283-313)."""
        n = C.c_size_t(0)
        capi.check(self.L.aa_parser_serialize_state(self.h, None, 0, C.byref(n)))
        buf = (C.c_uint8 * n.value)()
        capi.check(self.L.aa_parser_serialize_state(self.h, buf, n.value, C.byref(n)))
        return bytes(buf)

    def deserialize_state(self, blob):
        capi.check(self.L.aa_parser_deserialize_state(self.h, blob, len(blob)))

    def state_hash(self):
        """DecoderState::hash (decoder.cc:266-281)."""
        h = C.c_uint64()
        capi.check(self.L.aa_parser_state_hash(self.h, C.byref(h)))
        return h.value

    def probs(self):
        out = (C.c_uint8 * 1101)()
        capi.check(self.L.aa_parser_get_probs(self.h, out))
        return np.frombuffer(bytes(out), dtype=np.uint8)

    def segmentation(self):
        en, ab = C.c_int(), C.c_int()
        q, lf = (C.c_int8 * 4)(), (C.c_int8 * 4)()
        m = np.zeros(self.mbw * self.mbh, dtype=np.uint8)
        capi.check(self.L.aa_parser_get_segmentation(self.h, C.byref(en), C.byref(ab), q, lf, m.ctypes.data_as(C.POINTER(C.c_uint8))))
        return {"enabled": bool(en.value), "absolute": bool(ab.value), "quant": list(q), "lf": list(lf), "map": m.reshape(self.mbh, self.mbw)}

    def filter_adjustments(self):
        en = C.c_int(); r, m = (C.c_int8 * 4)(), (C.c_int8 * 4)()
        capi.check(self.L.aa_parser_get_filter_adjustments(self.h, C.byref(en), r, m))
        return {"enabled": bool(en.value), "ref": list(r), "mode": list(m)}


def serialize_host(header, ext, probs_before, mb, coeff_blocks, sub_modes=None, capacity=None):
    """A frame given as records written as VP8 bytes by one host core (aa_serialize_host: the statements of the GPU's token lanes and the
    host half's first partition; no device).  Arguments as Parser.parse / Parser.header_ext / Parser.probs / Parser.sub_modes return them."""
    L = capi.lib()
    hdr = Context._header_struct(header)
    x = capi.FrameHeaderExt.from_dict(ext)
    mbs = np.ascontiguousarray(mb, dtype=MB_INFO_DTYPE).reshape(-1)
    cf = np.ascontiguousarray(coeff_blocks, dtype=np.int16).reshape(-1, 16)
    hdr.num_coeff_blocks = len(cf)
    pb = np.ascontiguousarray(probs_before, dtype=np.uint8).reshape(-1)
    sm = None if sub_modes is None or len(sub_modes) == 0 else np.ascontiguousarray(sub_modes, dtype=np.uint8).reshape(-1)
    cap = int(capacity) if capacity is not None else 4096 + len(mbs) * 768
    out = np.zeros(cap, dtype=np.uint8)
    size = C.c_size_t()
    capi.check(L.aa_serialize_host(C.byref(hdr), C.byref(x), pb.ctypes.data_as(C.c_void_p), mbs.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p),
                                   None if sm is None else sm.ctypes.data_as(C.c_void_p), 0 if sm is None else len(sm), out.ctypes.data_as(C.c_void_p), cap, C.byref(size)))
    return out[:size.value].tobytes()


class Context:
    """One HIP device: compute + copy streams.  One per process in multi-GPU runs."""

    def __init__(self, device=0):
        self.L = capi.lib()
        self.h = C.c_void_p()
        capi.check(self.L.aa_ctx_create(device, C.byref(self.h)))
        self.device = device
        self._hash_keep = []                 # host arrays of outstanding hash calls

    def __del__(self):
        if getattr(self, "h", None):
            self.L.aa_ctx_destroy(self.h); self.h = None

    def sync(self):
        capi.check(self.L.aa_ctx_sync(self.h))

    def memory(self):
        """(free, total) bytes of this device's HBM right now."""
        f, t = C.c_size_t(), C.c_size_t()
        capi.check(self.L.aa_ctx_memory(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def set_memory_limit(self, nbytes):
        """HBM the context may take for its pools (default: 7/8 of what was free at creation)."""
        capi.check(self.L.aa_ctx_set_memory_limit(self.h, int(nbytes)))

    def set_host_share_ms(self, ms):
        """Key frames of big submit calls are parsed by host workers while that is expected to take no longer than `ms` (0: never)."""
        capi.check(self.L.aa_ctx_set_host_share_ms(self.h, float(ms)))

    def set_packed_coefficients(self, on=True):
        """Device-parsed frames store packed coefficients (mask word + non-zero values per block; expanded on the device when
        a frame is reconstructed) instead of dense blocks.  Before the context's first submit_frames only."""
        capi.check(self.L.aa_ctx_set_packed_coefficients(self.h, int(bool(on))))

    def set_lane_per_partition(self, on=True):
        """Frames with several DCT partitions may be entropy-decoded by one token lane per partition (lanes of one wave).  Before
        the context's first submit_frames only.  Simulated on the host; not yet run on a GPU."""
        capi.check(self.L.aa_ctx_set_lane_per_partition(self.h, int(bool(on))))

    def info(self):
        """What the context holds right now (aa_ctx_info): memory by kind, token-worker shape and occupancy."""
        st = capi.CtxInfo()
        capi.check(self.L.aa_ctx_get_info(self.h, C.byref(st)))
        d = {n: getattr(st, n) for n, _ in capi.CtxInfo._fields_}
        d["token_profile"] = list(st.token_profile)
        return d

    def pinned_alloc(self, nbytes):
        """Pinned host memory for asynchronous downloads (aa_pinned_alloc) -> address; free with pinned_free."""
        p = C.c_void_p()
        capi.check(self.L.aa_pinned_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def pinned_free(self, address):
        self.L.aa_pinned_free(C.c_void_p(address))

    def set_schedule(self, name):
        """"rows" (default): row-pipelined persistent kernels; "diagonal": one launch per anti-diagonal."""
        capi.check(self.L.aa_ctx_set_schedule(self.h, {"rows": 0, "diagonal": 1}[name]))

    def profile(self, enable):
        capi.check(self.L.aa_ctx_profile(self.h, int(enable)))

    def kernel_stats(self, reset=False):
        st = capi.KernelStats()
        capi.check(self.L.aa_ctx_kernel_stats(self.h, C.byref(st), int(reset)))
        return {n: getattr(st, n) for n, _ in capi.KernelStats._fields_}

    def compute_stream(self):
        return self.L.aa_ctx_compute_stream(self.h)

    ROUTES = {"auto": 0, "device": 2, "host": 4}

    def submit_frames(self, pairs, threads=0, defer_tokens=False, route="auto"):
        """Device-side entropy decode (aa_submit_frames): pairs = [(decoder, frame bytes), ...], frames of one decoder in
        stream order.  Host: frame-header pre-pass only; the macroblock headers and tokens are parsed on the GPU.
        -> frame index of every pair in its stream."""
        return self.submit_prepared(self.prepare_frames(pairs), threads, defer_tokens, route)

    def prepare_frames(self, pairs):
        """The ctypes argument block of submit_frames, reusable across calls with the same (decoder, bytes) pairs."""
        n = len(pairs)
        arr = (capi.FrameIn * n)()
        for i, (d, fr) in enumerate(pairs):
            arr[i].stream, arr[i].data, arr[i].size = d.h.value, fr, len(fr)
        return arr, (C.c_int * n)(), [fr for _, fr in pairs]      # (keeps the byte strings alive)

    def submit_prepared(self, prepared, threads=0, defer_tokens=False, route="auto"):
        """defer_tokens: two-phase form (AA_SUBMIT_DEFER_TOKENS) -- macroblock headers now, tokens at launch_tokens().
        route: "auto" (few streams -> host workers, many -> GPU lanes), "device", "host"."""
        arr, out, _keep = prepared
        capi.check(self.L.aa_submit_frames_ex(self.h, arr, len(arr), out, threads, (1 if defer_tokens else 0) | self.ROUTES[route]))
        return list(out)

    def launch_tokens(self, max_batches=0):
        """Second phase of the oldest `max_batches` deferred batches (0: all) -> how many were launched."""
        n = C.c_int()
        capi.check(self.L.aa_launch_tokens(self.h, max_batches, C.byref(n)))
        return n.value

    def download_batch_async(self, decoders, frame_indices, dst_ptr, stride):
        """aa_download_batch_async: frame frame_indices[i] of decoders[i] -> dst_ptr + i * stride (pinned host memory), one gather
        kernel + one copy for the lot; valid after download_wait() / sync()."""
        n = len(decoders)
        arr = (C.c_void_p * n)(*[d.h for d in decoders])
        idx = (C.c_int * n)(*frame_indices)
        capi.check(self.L.aa_download_batch_async(self.h, arr, n, idx, C.c_void_p(dst_ptr), stride))

    def download_wait(self, max_in_flight=None):
        """aa_ctx_download_wait: every batched download queued so far has arrived; with max_in_flight: only until at most that many are
        still on their way (aa_ctx_download_wait_until: a ring of r destination buffers waits with r - 1 before it reuses one)."""
        if max_in_flight is None:
            capi.check(self.L.aa_ctx_download_wait(self.h))
        else:
            capi.check(self.L.aa_ctx_download_wait_until(self.h, int(max_in_flight)))

    # format -> (AA_RGB_* code, torch dtype, channels of an HWC format / None for CHW)
    RGB_FORMATS = {"rgb24": (capi.AA_RGB_U8_HWC3, "uint8", 3), "rgba": (capi.AA_RGB_U8_HWC4, "uint8", 4),
                   "chw_u8": (capi.AA_RGB_U8_CHW, "uint8", None), "chw_f16": (capi.AA_RGB_F16_CHW, "float16", None),
                   "chw_bf16": (capi.AA_RGB_BF16_CHW, "bfloat16", None), "chw_f32": (capi.AA_RGB_F32_CHW, "float32", None)}

    def to_rgb(self, decoders, frame_indices, format="rgb24", mean=None, std=None, out=None):
        """Frame frame_indices[i] of decoders[i] as RGB on this context's device, all in one kernel (aa_render_rgb_async): the
        display rectangle, SMPTE 170M limited range, as the reference's display shader shows it.
        -> torch tensor (N, H, W, 3|4) uint8 for "rgb24" / "rgba", (N, 3, H, W) for "chw_u8" / "chw_f16" / "chw_bf16" / "chw_f32"
        (float formats: (rgb / 255 - mean[c]) / std[c]).  The result is ordered on torch.cuda.current_stream(): torch ops may use it
        without a sync.  out: a tensor of that shape, or a list of per-frame tensors ((H, W, C) / (3, H, W); frames of different
        display sizes need this form); views with padded rows are accepted, the innermost dimension must be contiguous."""
        import torch
        if format not in self.RGB_FORMATS:
            raise ValueError("unknown RGB format %r (one of %s)" % (format, ", ".join(self.RGB_FORMATS)))
        code, dtype_name, hwc = self.RGB_FORMATS[format]
        dtype = getattr(torch, dtype_name)
        n = len(decoders)
        if n == 0 or len(frame_indices) != n:
            raise ValueError("to_rgb: need as many frame indices as decoders, and at least one")
        device = torch.device("cuda", self.device)

        def frame_shape(d):
            return (d.height, d.width, hwc) if hwc else (3, d.height, d.width)

        if isinstance(out, (list, tuple)):
            if len(out) != n:
                raise ValueError("to_rgb: out has %d tensors for %d frames" % (len(out), n))
            frames = result = list(out)
        else:
            shapes = {frame_shape(d) for d in decoders}
            if len(shapes) != 1:
                raise ValueError("to_rgb: frames of different display sizes need out= as a list of tensors")
            shape = (n,) + shapes.pop()
            if out is None:
                out = torch.empty(shape, dtype=dtype, device=device)
            elif tuple(out.shape) != shape:
                raise ValueError("to_rgb: out has shape %s, expected %s" % (tuple(out.shape), shape))
            result, frames = out, list(out.unbind(0))
        targets = (capi.RgbTarget * n)()
        for i, (t, d) in enumerate(zip(frames, decoders)):
            if tuple(t.shape) != frame_shape(d):
                raise ValueError("to_rgb: out[%d] has shape %s, expected %s" % (i, tuple(t.shape), frame_shape(d)))
            if t.dtype != dtype or t.device != device:
                raise ValueError("to_rgb: out[%d] is %s on %s, expected %s on %s" % (i, t.dtype, t.device, dtype, device))
            es = t.element_size()
            if hwc and (t.stride(2) != 1 or t.stride(1) != hwc):
                raise ValueError("to_rgb: out[%d]: the pixels of a row must be contiguous" % i)
            if not hwc and t.stride(2) != 1:
                raise ValueError("to_rgb: out[%d]: the rows must be contiguous" % i)
            targets[i].dst = t.data_ptr()
            targets[i].row_stride = t.stride(0 if hwc else 1) * es
            targets[i].plane_stride = 0 if hwc else t.stride(0) * es
        arr = (C.c_void_p * n)(*[d.h for d in decoders])
        idx = (C.c_int * n)(*frame_indices)
        m = None if mean is None else (C.c_double * 3)(*[float(x) for x in mean])
        sd = None if std is None else (C.c_double * 3)(*[float(x) for x in std])
        cur = torch.cuda.current_stream(device)
        compute = None
        if not cur.cuda_stream:
            # torch's default stream is HIP's null stream, whose handle (0) means "no consumer stream" to the C call: the same two
            # waits are made through torch's own events instead
            compute = torch.cuda.ExternalStream(self.compute_stream(), device=device)
            compute.wait_stream(cur)
        capi.check(self.L.aa_render_rgb_async(self.h, arr, n, idx, code, targets, m, sd, C.c_void_p(cur.cuda_stream or None)))
        if compute is not None:
            cur.wait_stream(compute)
        return result

    QUALITY_PLANES = {"y": capi.AA_QUALITY_Y, "yuv": capi.AA_QUALITY_YUV}

    def quality(self, decoders, frame_indices, originals, planes="y", out=None):
        """Frame frame_indices[i] of decoders[i] scored against originals[i] on this context's device (aa_quality_batch_async):
        BaseRaster::quality -- x264's SSIM, the value aa_ssim_host gives, bit for bit -- and the sum of squared differences, per plane
        over the PADDED planes.  planes: "y" or "yuv".  originals[i]: a tuple (y, u, v) of uint8 device tensors of the padded plane
        shapes (u, v may be None for "y"; views with padded rows are accepted, the innermost stride must be 1), or a pair
        (decoder, frame_index) for decoded against decoded.
        -> Quality(ssim: float64 (N, P), sse: int64 (N, P)), ordered on torch.cuda.current_stream() like to_rgb's result; out: a pair
        of such tensors (contiguous) to write into."""
        import torch
        if planes not in self.QUALITY_PLANES:
            raise ValueError("quality: planes must be \"y\" or \"yuv\", not %r" % (planes,))
        np_ = self.QUALITY_PLANES[planes]
        n = len(decoders)
        if n == 0 or len(frame_indices) != n or len(originals) != n:
            raise ValueError("quality: need as many frame indices and originals as decoders, and at least one")
        device = torch.device("cuda", self.device)
        if out is None:
            ssim = torch.empty((n, np_), dtype=torch.float64, device=device)
            sse = torch.empty((n, np_), dtype=torch.int64, device=device)
        else:
            ssim, sse = out
            for name, t, dt in (("ssim", ssim, torch.float64), ("sse", sse, torch.int64)):
                if tuple(t.shape) != (n, np_) or t.dtype != dt or t.device != device or not t.is_contiguous():
                    raise ValueError("quality: out %s must be a contiguous %s tensor of shape %s on %s" % (name, dt, (n, np_), device))
        refs = (capi.QualityRef * n)()
        keep = []
        for i, (d, o) in enumerate(zip(decoders, originals)):
            if len(o) == 2 and isinstance(o[0], Decoder):
                od, ofi = o
                if (od.padded_width, od.padded_height) != (d.padded_width, d.padded_height):
                    raise ValueError("quality: originals[%d] is a frame of %dx%d padded, expected %dx%d"
                                     % (i, od.padded_width, od.padded_height, d.padded_width, d.padded_height))
                if od.ctx is not self:
                    raise ValueError("quality: originals[%d] is a decoder of another context" % i)
                if not 0 <= ofi < od.frame_count():
                    raise ValueError("quality: originals[%d]: bad frame index %d" % (i, ofi))
                refs[i].y, refs[i].u, refs[i].v = od.raster_device_pointers(ofi)
                refs[i].y_stride, refs[i].uv_stride = d.padded_width, d.padded_width // 2
                continue
            if len(o) != 3:
                raise ValueError("quality: originals[%d] must be (y, u, v) or (decoder, frame_index)" % i)
            ptrs, strides = [None] * 3, [0, 0, 0]
            for p, t in enumerate(o):
                if p >= np_:
                    break
                shape = (d.padded_height, d.padded_width) if p == 0 else (d.padded_height // 2, d.padded_width // 2)
                if t is None:
                    raise ValueError("quality: originals[%d]: plane %d is None" % (i, p))
                if tuple(t.shape) != shape:
                    raise ValueError("quality: originals[%d]: plane %d has shape %s, expected %s" % (i, p, tuple(t.shape), shape))
                if t.dtype != torch.uint8 or t.device != device:
                    raise ValueError("quality: originals[%d]: plane %d is %s on %s, expected torch.uint8 on %s" % (i, p, t.dtype, t.device, device))
                if t.stride(1) != 1 or t.stride(0) < shape[1]:
                    raise ValueError("quality: originals[%d]: plane %d: the rows must be contiguous and must not overlap" % (i, p))
                ptrs[p], strides[p] = t.data_ptr(), t.stride(0)
                keep.append(t)
            if np_ == 3 and strides[1] != strides[2]:
                raise ValueError("quality: originals[%d]: u and v must have the same row stride" % i)
            refs[i].y, refs[i].u, refs[i].v = ptrs
            refs[i].y_stride, refs[i].uv_stride = strides[0], strides[1]
        arr = (C.c_void_p * n)(*[d.h for d in decoders])
        idx = (C.c_int * n)(*frame_indices)
        cur = torch.cuda.current_stream(device)
        compute = None
        if not cur.cuda_stream:
            # (the null stream's handle means "no consumer stream" to the C call: the two waits are made through torch, as in to_rgb)
            compute = torch.cuda.ExternalStream(self.compute_stream(), device=device)
            compute.wait_stream(cur)
        capi.check(self.L.aa_quality_batch_async(self.h, arr, n, idx, refs, np_, C.c_void_p(ssim.data_ptr()), C.c_void_p(sse.data_ptr()),
                                                 C.c_void_p(cur.cuda_stream or None)))
        if compute is not None:
            cur.wait_stream(compute)
        return Quality(ssim, sse)

    def _target_planes(self, what, i, d, t):
        """targets[i] of a rebase / re-encode, checked -> (y, u, v) device tensors of decoder d's padded plane shapes."""
        import torch
        device = torch.device("cuda", self.device)
        pw, ph = d.padded_width, d.padded_height
        shapes = [(ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2)]
        if isinstance(t, torch.Tensor):
            if t.dtype != torch.uint8 or t.device != device or not t.is_contiguous() or t.numel() != pw * ph * 3 // 2:
                raise ValueError("%s: targets[%d] must be a contiguous torch.uint8 tensor of %d bytes on %s" % (what, i, pw * ph * 3 // 2, device))
            flat = t.reshape(-1)
            t = (flat[:pw * ph].view(shapes[0]), flat[pw * ph:pw * ph * 5 // 4].view(shapes[1]), flat[pw * ph * 5 // 4:].view(shapes[2]))
        if len(t) != 3:
            raise ValueError("%s: targets[%d] must be a tensor or (y, u, v)" % (what, i))
        for p, (pl, shape) in enumerate(zip(t, shapes)):
            if tuple(pl.shape) != shape or pl.dtype != torch.uint8 or pl.device != device or pl.stride(1) != 1 or pl.stride(0) < shape[1]:
                raise ValueError("%s: targets[%d]: plane %d must be torch.uint8 of shape %s on %s with contiguous rows" % (what, i, p, shape, device))
        if t[1].stride(0) != t[2].stride(0):
            raise ValueError("%s: targets[%d]: u and v must have the same row stride" % (what, i))
        return t

    @staticmethod
    def _header_struct(header):
        hdr = FrameHeader()
        for name, _ in FrameHeader._fields_:
            if name == "quant":
                for sgm in range(4):
                    for k in range(6):
                        hdr.quant[sgm][k] = header["quant"][sgm][k]
            else:
                setattr(hdr, name, header[name])
        return hdr

    def rebase(self, decoders, headers, mbs, targets, records=True):
        """The rebase (aa_rebase_batch; Encoder::update_residues, reencode.cc:236-303), one new frame per decoder: headers[i] (a dict
        as Parser.parse / frame_header return it: quant[0] are the factors divided by, key_frame 0) and mbs[i] (the prediction frame's
        records: modes, references and vectors are kept) with residues recomputed so that the frame decodes to targets[i] from
        decoders[i]'s current references.  targets[i]: (y, u, v) uint8 device tensors of the padded plane shapes, edge-extended by the
        caller (rows may be padded), or one contiguous uint8 device tensor holding the three padded planes back to back.
        -> per job (frame_index, mb [mbh, mbw], coeff_blocks [n, 16]) in the shapes Decoder.read_records returns; the frame is
        appended to its decoder and is decoded like any other (Context.decode_batch).  Synchronous.
        records=False (aa_rebase_device_batch): the new frame's records are compacted on the device and stay there -- nothing but a few
        count words comes down -- and the result per job is (frame_index, num_coeff_blocks); Decoder.read_records gives the records
        to whoever wants them on the host, Context.serialize_frames and Context.decode_batch take the frame where it lies."""
        import torch
        n = len(decoders)
        if n == 0 or len(headers) != n or len(mbs) != n or len(targets) != n:
            raise ValueError("rebase: need as many headers, records and targets as decoders, and at least one")
        device = torch.device("cuda", self.device)
        if not records:
            jobs = (capi.RebaseDeviceJob * n)()
            keep = []
            for i, (d, header, mb, t) in enumerate(zip(decoders, headers, mbs, targets)):
                t = self._target_planes("rebase", i, d, t)
                hdr = self._header_struct(header)
                rec = np.ascontiguousarray(mb, dtype=MB_INFO_DTYPE).reshape(-1)
                if len(rec) != hdr.mb_width * hdr.mb_height:
                    raise ValueError("rebase: mbs[%d] holds %d records, the header says %d" % (i, len(rec), hdr.mb_width * hdr.mb_height))
                j = jobs[i]
                j.stream, j.hdr, j.mbs = d.h, C.pointer(hdr), rec.ctypes.data_as(C.c_void_p)
                j.target.y, j.target.u, j.target.v = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
                j.target.y_stride, j.target.uv_stride = t[0].stride(0), t[1].stride(0)
                keep.append((hdr, rec, t))
            torch.cuda.current_stream(device).synchronize()
            capi.check(self.L.aa_rebase_device_batch(self.h, jobs, n))
            return [(jobs[i].frame_index, jobs[i].num_coeff_blocks) for i in range(n)]
        jobs = (capi.RebaseJob * n)()
        keep, outs = [], []
        for i, (d, header, mb, t) in enumerate(zip(decoders, headers, mbs, targets)):
            t = self._target_planes("rebase", i, d, t)
            hdr = self._header_struct(header)
            nmb = hdr.mb_width * hdr.mb_height
            rec = np.ascontiguousarray(mb, dtype=MB_INFO_DTYPE).reshape(-1)
            if len(rec) != nmb:
                raise ValueError("rebase: mbs[%d] holds %d records, the header says %d" % (i, len(rec), nmb))
            mb_out = np.zeros(nmb, dtype=MB_INFO_DTYPE)
            cf = np.zeros((nmb * 25, 16), dtype=np.int16)
            j = jobs[i]
            j.stream, j.hdr, j.mbs = d.h, C.pointer(hdr), rec.ctypes.data_as(C.c_void_p)
            j.target.y, j.target.u, j.target.v = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
            j.target.y_stride, j.target.uv_stride = t[0].stride(0), t[1].stride(0)
            j.mbs_out, j.coeffs_out, j.coeff_capacity_blocks = mb_out.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), len(cf)
            keep.append((hdr, rec, t))
            outs.append((mb_out, cf, hdr.mb_width, hdr.mb_height))
        torch.cuda.current_stream(device).synchronize()      # (the targets are ready; the call itself waits for its kernels)
        capi.check(self.L.aa_rebase_batch(self.h, jobs, n))
        return [(jobs[i].frame_index, mb_out.reshape(mbh, mbw), cf[:jobs[i].num_coeff_blocks].copy()) for i, (mb_out, cf, mbw, mbh) in enumerate(outs)]

    def rebase_timing(self):
        """The last rebase of this context (aa_rebase_last_timing), ms: call, upload + kernels, download, host records, append (for a
        rebase with records=False: the download is the count words, the host records are 0, the append is bookkeeping)."""
        out = (C.c_double * 5)()
        capi.check(self.L.aa_rebase_last_timing(self.h, out))
        return dict(zip(("call_ms", "kernels_ms", "download_ms", "records_ms", "append_ms"), out))

    def reencode_as_inter(self, decoders, headers, targets, quality="best", append=True, records=True):
        """The re-encode (aa_reencode_batch; Encoder::reencode_as_interframe, reencode.cc:38-129), one new frame per decoder: targets[i]
        -- a chunk's first picture -- encoded as an inter frame predicted from decoders[i]'s current last reference, every macroblock's
        mode chosen as the reference's encoder chooses it (quality: "best" or "rt", for all jobs or one per job).  headers[i] and
        targets[i] as for rebase.  -> per job (frame_index, mb [mbh, mbw], coeff_blocks [n, 16]) as rebase returns them; with append
        False nothing is appended and frame_index is -1 (the records go through Decoder.append_records when the frame is final).
        Synchronous.
        records=False (aa_reencode_device_batch): the new frame's records are compacted on the device and stay there, as with
        rebase( records=False ) -- the result per job is (frame_index, num_coeff_blocks).  Such a frame is always appended: together
        with append=False this raises ValueError."""
        return self._decide_frames("reencode_as_inter", self.L.aa_reencode_batch, self.L.aa_reencode_device_batch, decoders, headers, targets, quality, append, records)

    def encode_frames(self, decoders, headers, targets, quality="best", append=True, records=True, two_pass=False):
        """The forward encoder (aa_encode_batch; Encoder::encode_with_quantizer, encoder.cc:559-575: xc-enc -i y4m -y QI -q best|rt), one
        new frame per decoder: targets[i] encoded as a key frame where headers[i]["key_frame"] is set (encode_raster<KeyFrame>; needs
        no reference and no earlier frame) and otherwise as an inter frame predicted from decoders[i]'s current last reference
        (encode_raster<InterFrame>), every macroblock's mode, vector and coefficients as the reference's single-pass encoder chooses
        them (quality: "best" or "rt", for all jobs or one per job).  One call may mix kinds, sizes and qualities.  headers[i] -- the
        caller's: q_index and quant (aa.quant_factors), loop filter fields, refresh flags -- and targets[i] as for rebase.  -> per job
        (frame_index, mb [mbh, mbw], coeff_blocks [n, 16]) as reencode_as_inter returns them; with append False nothing is appended
        and frame_index is -1.  The frames go on to lf_search_decode / decode_batch and serialize_frames( optimise=True ).  Synchronous.
        records=False (aa_encode_device_batch): the new frame's records are compacted on the device and stay there -- the result per
        job is (frame_index, num_coeff_blocks).  Such a frame is always appended: together with append=False this raises ValueError.
        two_pass (one flag or one per job; aa_encode_two_pass_batch / aa_encode_two_pass_device_batch: xc-enc --two-pass): a KEY job
        whose flag is set runs the reference's second pass behind the first -- the decision again with trellis quantisation and
        check_reset_y2 (encode_intra.cc:409-439) -- and its records are the second pass's; inter jobs are untouched.  Where any flag is
        set every job's result has one more element: the FIRST pass's token_prob_update, uint8 [2112] (1056 flags, 1056 values; zero
        for a job without a second pass), which serialize_frames( optimise=True, first_pass_updates=... ) keeps wherever the second
        pass makes no update, as the reference does.  With no flag set the call and its results are exactly those without the argument."""
        flags = [bool(f) for f in two_pass] if isinstance(two_pass, (list, tuple, np.ndarray)) else [bool(two_pass)] * len(decoders)
        if len(flags) != len(decoders):
            raise ValueError("encode_frames: two_pass is one flag or one per job")
        if not any(flags):
            return self._decide_frames("encode_frames", self.L.aa_encode_batch, self.L.aa_encode_device_batch, decoders, headers, targets, quality, append, records)
        n = len(decoders)
        which = np.array(flags, dtype=np.uint8)
        updates = np.zeros((n, capi.TWO_PASS_UPDATES), dtype=np.uint8)
        extra = (which.ctypes.data_as(C.c_void_p), updates.ctypes.data_as(C.c_void_p))
        out = self._decide_frames("encode_frames", self.L.aa_encode_two_pass_batch, self.L.aa_encode_two_pass_device_batch, decoders, headers, targets, quality, append,
                                  records, extra)
        return [r + (updates[i].copy(),) for i, r in enumerate(out)]

    def _decide_frames(self, who, host_call, device_call, decoders, headers, targets, quality, append, records, extra=()):
        """reencode_as_inter and encode_frames: the same jobs into two pairs of ABI calls (extra: what a call takes behind its jobs)."""
        import torch
        n = len(decoders)
        if n == 0 or len(headers) != n or len(targets) != n:
            raise ValueError(who + ": need as many headers and targets as decoders, and at least one")
        qualities = [quality] * n if isinstance(quality, str) else list(quality)
        if len(qualities) != n or any(q not in ("best", "rt") for q in qualities):
            raise ValueError(who + ": quality is \"best\" or \"rt\", one for all jobs or one per job")
        if not records:
            if not append:
                raise ValueError(who + ": records=False keeps the frame on the device, where it is always appended; append=False needs records=True")
            jobs = (capi.ReencodeDeviceJob * n)()
            keep = []
            for i, (d, header, t) in enumerate(zip(decoders, headers, targets)):
                t = self._target_planes(who, i, d, t)
                hdr = self._header_struct(header)
                j = jobs[i]
                j.stream, j.hdr, j.quality = d.h, C.pointer(hdr), (1 if qualities[i] == "rt" else 0)
                j.target.y, j.target.u, j.target.v = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
                j.target.y_stride, j.target.uv_stride = t[0].stride(0), t[1].stride(0)
                keep.append((hdr, t))
            torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()
            capi.check(device_call(self.h, jobs, n, *extra))
            return [(jobs[i].frame_index, jobs[i].num_coeff_blocks) for i in range(n)]
        jobs = (capi.ReencodeJob * n)()
        keep, outs = [], []
        for i, (d, header, t) in enumerate(zip(decoders, headers, targets)):
            t = self._target_planes(who, i, d, t)
            hdr = self._header_struct(header)
            nmb = hdr.mb_width * hdr.mb_height
            mb_out = np.zeros(nmb, dtype=MB_INFO_DTYPE)
            cf = np.zeros((nmb * 25, 16), dtype=np.int16)
            j = jobs[i]
            j.stream, j.hdr = d.h, C.pointer(hdr)
            j.target.y, j.target.u, j.target.v = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
            j.target.y_stride, j.target.uv_stride = t[0].stride(0), t[1].stride(0)
            j.quality, j.append = (1 if qualities[i] == "rt" else 0), int(bool(append))
            j.mbs_out, j.coeffs_out, j.coeff_capacity_blocks = mb_out.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), len(cf)
            keep.append((hdr, t))
            outs.append((mb_out, cf, hdr.mb_width, hdr.mb_height))
        torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()      # (the targets are ready; the call itself waits for its kernel)
        capi.check(host_call(self.h, jobs, n, *extra))
        return [(jobs[i].frame_index, mb_out.reshape(mbh, mbw), cf[:jobs[i].num_coeff_blocks].copy()) for i, (mb_out, cf, mbw, mbh) in enumerate(outs)]

    def serialize_frames(self, decoders, frame_indices, headers, exts, probs_before=None, advance_state=False, capacity=None, optimise=False, sub_modes=None, details=False,
                         first_pass_updates=None):
        """The serialisation (aa_serialize_batch; Frame::serialize, serializer.cc:388-829): frame frame_indices[i] of decoders[i], held as
        records (parsed, rebased, re-encoded or appended), written as a VP8 frame with the header headers[i] (a dict as Parser.parse /
        frame_header return it) and exts[i] (a dict as Parser.header_ext returns it) -- DCT partitions on the GPU, first partition on the
        host.  probs_before: per job 1101 bytes as Parser.probs() returns them, or None for the decoder's current tables (None for all:
        every job); advance_state (one flag or one per job): the decoder's DecoderState then follows the written frame as if it had
        parsed it.  capacity: bytes per frame (default: 4 KiB + 768 bytes per macroblock, twice a raw frame; a frame
        that takes more is refused with the size it needs in the message).  sub_modes: per job None or the
        SPLITMV sub-block modes of the frame the records came from (Parser.sub_modes): without them the frame parses to the same records
        but is not necessarily the original's bytes.  optimise: the reference's probability passes (optimize_prob_skip,
        optimize_interframe_probs, optimize_probability_tables) run on the GPU first and decide prob_skip_false, the three reference
        probabilities and the token probability updates, whatever exts[i] says of them.  -> [bytes], or with details [(bytes, the
        header extension as written, the branch counts the passes used: uint32 [2120], None without optimise)].  Synchronous.
        first_pass_updates (aa_serialize_two_pass_batch): per job None or the uint8 [2112] encode_frames( two_pass=True ) returned for
        the frame -- with optimise, wherever the probability pass decides no update the first pass's update is kept, as the reference's
        two-pass encoder leaves its header; None (for all jobs) is exactly the call without the argument.
        (Decoder.serialize is the decoder's STATE in the reference's format; this is a frame.)"""
        n = len(decoders)
        if n == 0 or len(frame_indices) != n or len(headers) != n or len(exts) != n:
            raise ValueError("serialize_frames: need as many frame indices, headers and header extensions as decoders, and at least one")
        before = list(probs_before) if probs_before is not None else [None] * n
        advance = list(advance_state) if isinstance(advance_state, (list, tuple)) else [advance_state] * n
        caps = list(capacity) if isinstance(capacity, (list, tuple)) else [capacity] * n
        subs = list(sub_modes) if sub_modes is not None else [None] * n
        if len(before) != n or len(advance) != n or len(caps) != n or len(subs) != n:
            raise ValueError("serialize_frames: per-job arguments must be one per decoder")
        first = None
        if first_pass_updates is not None:
            if len(first_pass_updates) != n:
                raise ValueError("serialize_frames: first_pass_updates must be one per decoder")
            first = np.zeros((n, capi.TWO_PASS_UPDATES), dtype=np.uint8)
            for i, u in enumerate(first_pass_updates):
                if u is None:
                    continue
                u = np.ascontiguousarray(u, dtype=np.uint8).reshape(-1)
                if len(u) != capi.TWO_PASS_UPDATES:
                    raise ValueError("serialize_frames: first_pass_updates[%d] holds %d bytes, not %d" % (i, len(u), capi.TWO_PASS_UPDATES))
                first[i] = u
        jobs = (capi.SerializeJob * n)()
        keep, outs = [], []
        for i, d in enumerate(decoders):
            hdr = self._header_struct(headers[i])
            ext = capi.FrameHeaderExt.from_dict(exts[i])
            nmb = hdr.mb_width * hdr.mb_height
            cap = int(caps[i]) if caps[i] is not None else 4096 + nmb * 768
            out = np.zeros(max(cap, 1), dtype=np.uint8)
            pb = None if before[i] is None else np.ascontiguousarray(before[i], dtype=np.uint8).reshape(-1)
            if pb is not None and len(pb) != 1101:
                raise ValueError("serialize_frames: probs_before[%d] holds %d bytes, not 1101" % (i, len(pb)))
            j = jobs[i]
            j.stream, j.frame_index, j.hdr, j.ext = d.h, int(frame_indices[i]), C.pointer(hdr), C.pointer(ext)
            j.optimise, j.advance_state = int(bool(optimise)), int(bool(advance[i]))
            j.probs_before = None if pb is None else pb.ctypes.data_as(C.c_void_p)
            j.out, j.capacity = out.ctypes.data_as(C.c_void_p), cap
            sm = None if subs[i] is None or len(subs[i]) == 0 else np.ascontiguousarray(subs[i], dtype=np.uint8).reshape(-1)
            j.sub_modes, j.num_sub_modes = (None, 0) if sm is None else (sm.ctypes.data_as(C.c_void_p), len(sm))
            cnt = np.zeros(2120, dtype=np.uint32) if (optimise and details) else None
            j.counts_out = None if cnt is None else cnt.ctypes.data_as(C.c_void_p)
            keep.append((hdr, ext, pb, sm, cnt))
            outs.append(out)
        if first is None:
            capi.check(self.L.aa_serialize_batch(self.h, jobs, n))
        else:
            capi.check(self.L.aa_serialize_two_pass_batch(self.h, jobs, n, first.ctypes.data_as(C.c_void_p)))
        if details:
            return [(outs[i][:jobs[i].size].tobytes(), keep[i][1].as_dict(), keep[i][4]) for i in range(n)]
        return [outs[i][:jobs[i].size].tobytes() for i in range(n)]

    def serialize_timing(self):
        """The last serialisation of this context (aa_serialize_last_timing), ms: call, upload + token kernel, sizes + partitions down,
        host first partitions (beside the kernel), assembly + copy + state advance."""
        out = (C.c_double * 5)()
        capi.check(self.L.aa_serialize_last_timing(self.h, out))
        return dict(zip(("call_ms", "kernel_ms", "download_ms", "first_partition_ms", "assemble_ms"), out))

    def reencode_timing(self):
        """The last re-encode of this context (aa_reencode_last_timing), ms: call, upload + kernel, download, host records, append (for a
        re-encode with records=False: the download is the count and row words, the host records are 0, the append is bookkeeping)."""
        out = (C.c_double * 5)()
        capi.check(self.L.aa_reencode_last_timing(self.h, out))
        return dict(zip(("call_ms", "kernels_ms", "download_ms", "records_ms", "append_ms"), out))

    def encode_timing(self):
        """The last encode_frames of this context (aa_encode_last_timing), ms: as reencode_timing."""
        out = (C.c_double * 5)()
        capi.check(self.L.aa_encode_last_timing(self.h, out))
        return dict(zip(("call_ms", "kernels_ms", "download_ms", "records_ms", "append_ms"), out))

    def _size_jobs(self, who, job_type, decoders, targets, key_frame, quality, carry):
        """estimate_frame_sizes and target_size_q: what their jobs share -> (jobs, what must stay alive)"""
        n = len(decoders)
        if len(targets) != n:
            raise ValueError(who + ": need as many targets as decoders")
        keys = list(key_frame) if isinstance(key_frame, (list, tuple)) else [key_frame] * n
        qualities = [quality] * n if isinstance(quality, str) else list(quality)
        carries = [capi.estimate_carry()] * n if carry is None else ([tuple(carry)] * n if n and not isinstance(carry[0], (list, tuple, np.ndarray)) else [tuple(c) for c in carry])
        if len(keys) != n or len(qualities) != n or len(carries) != n or any(len(c) != 4 for c in carries):
            raise ValueError(who + ": key_frame, quality and carry are one for all jobs or one per job; a carry is four bytes")
        if any(q not in ("best", "rt") for q in qualities):
            raise ValueError(who + ": quality is \"best\" or \"rt\", one for all jobs or one per job")
        jobs = (job_type * max(n, 1))()
        keep = []
        for i, (d, t) in enumerate(zip(decoders, targets)):
            t = self._target_planes(who, i, d, t)
            j = jobs[i]
            j.stream, j.key_frame, j.quality = d.h, int(bool(keys[i])), (1 if qualities[i] == "rt" else 0)
            j.target.y, j.target.u, j.target.v = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
            j.target.y_stride, j.target.uv_stride = t[0].stride(0), t[1].stride(0)
            j.carry = (C.c_uint8 * 4)(*[int(x) for x in carries[i]])
            keep.append(t)
        if n:
            import torch
            torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()      # (the targets are ready; the call itself waits for its kernels)
        return jobs, keep

    def estimate_frame_sizes(self, decoders, targets, q_indices, key_frame=False, quality="best", carry=None):
        """The frame-size estimate (aa_estimate_size_batch; Encoder::estimate_frame_size, size_estimation.cc: the number xc-enc -y prints as
        [estimated size=N]), one picture per decoder: targets[i] (as encode_frames takes them) encoded at q_indices[i] (one for all or
        one per job) as a frame of a quarter of the size in each direction made of every fourth macroblock -- a key estimate where
        key_frame is set, else predicted from decoders[i]'s current last reference under its current tables -- and that frame's serialised
        size times 16.  carry: None (aa.estimate_carry()), one for all or one per job: four bytes, see aa_estimate_size_job.
        -> [(size, carry after)].  Nothing is appended, no decoder changes.  Synchronous."""
        n = len(decoders)
        jobs, keep = self._size_jobs("estimate_frame_sizes", capi.EstimateSizeJob, decoders, targets, key_frame, quality, carry)
        qs = list(q_indices) if isinstance(q_indices, (list, tuple, np.ndarray)) else [q_indices] * n
        if len(qs) != n:
            raise ValueError("estimate_frame_sizes: q_indices is one for all jobs or one per job")
        for i in range(n):
            jobs[i].q_index = int(qs[i])
        capi.check(self.L.aa_estimate_size_batch(self.h, jobs, n))
        return [(int(jobs[i].size_out), tuple(jobs[i].carry)) for i in range(n)]

    def target_size_q(self, decoders, targets, target_sizes, q_lo=4, q_hi=127, key_frame=False, quality="best", carry=None):
        """The quantiser for a target frame size (aa_target_size_batch; Encoder::encode_with_target_size, encoder.cc:592-629: xc-enc -F),
        one picture per decoder: the reference's bisection over q_lo..q_hi (aa.target_size_range; one for all or one per job) with
        estimate_frame_sizes' estimate, all jobs moving together in rounds of one candidate each, at most 7 (8 from a range of all 128 indices).  -> [(q_index, [(q, size)]
        visited in order, carry after)]; the chosen index goes into the header encode_frames is given.  Nothing is appended, no decoder
        changes.  Synchronous."""
        n = len(decoders)
        jobs, keep = self._size_jobs("target_size_q", capi.TargetSizeJob, decoders, targets, key_frame, quality, carry)
        sizes = list(target_sizes) if isinstance(target_sizes, (list, tuple, np.ndarray)) else [target_sizes] * n
        los = list(q_lo) if isinstance(q_lo, (list, tuple)) else [q_lo] * n
        his = list(q_hi) if isinstance(q_hi, (list, tuple)) else [q_hi] * n
        if len(sizes) != n or len(los) != n or len(his) != n:
            raise ValueError("target_size_q: target_sizes, q_lo and q_hi are one for all jobs or one per job")
        for i in range(n):
            jobs[i].target_size, jobs[i].q_lo, jobs[i].q_hi = int(sizes[i]), int(los[i]), int(his[i])
        capi.check(self.L.aa_target_size_batch(self.h, jobs, n))
        return [(jobs[i].q_index, [(jobs[i].visited_q[k], int(jobs[i].visited_size[k])) for k in range(jobs[i].estimates)], tuple(jobs[i].carry)) for i in range(n)]

    def set_target_size_round(self, jobs_per_slice=0):
        """Jobs per slice of a round of estimate_frame_sizes / target_size_q (0: by memory) -- aa_ctx_set_target_size_round."""
        capi.check(self.L.aa_ctx_set_target_size_round(self.h, int(jobs_per_slice)))

    def target_size_timing(self):
        """The last estimate_frame_sizes or target_size_q of this context (aa_target_size_last_timing), ms: the call (wall clock), then
        summed over rounds and slices the uploads with the decision kernels, k_estimate_tokens, the results coming down (HIP events),
        the host's first partitions with the rule (wall clock); and the number of rounds."""
        out = (C.c_double * 6)()
        capi.check(self.L.aa_target_size_last_timing(self.h, out))
        return dict(zip(("call_ms", "decisions_ms", "tokens_ms", "download_ms", "host_ms", "rounds"), out))

    def set_reencode_slots(self, slots):
        """Macroblocks of an anti-diagonal per round of the re-encode kernel and of the forward encoder's two (aa_ctx_set_reencode_slots:
        1..16, default 16)."""
        capi.check(self.L.aa_ctx_set_reencode_slots(self.h, int(slots)))

    LF_MEASURES = {"ssim": capi.AA_LF_MEASURE_SSIM, "sse": capi.AA_LF_MEASURE_SSE}

    def lf_search_decode(self, decoders, frame_indices, originals, level_lo=0, level_hi=63, measure="ssim"):
        """The loop-filter level search of appended frames, and their decode (aa_lf_search_decode_batch; the last statement of
        Encoder::reencode_as_interframe): frame frame_indices[i] is decoders[i]'s next frame to decode, held as records (append_records,
        rebase, reencode_as_inter, with records on the host or on the device) under any provisional level.  originals[i]: the target the
        frame stands for, as reencode_as_inter takes it (the luma plane is read).  level_lo / level_hi: one for all jobs or one per job.
        measure: "ssim" (x264's SSIM of the padded luma, Context.quality's value) or "sse" (1 - mean squared error / 255^2).
        -> per job (best_level, best_score, evaluated); afterwards every frame is decoded, filtered with its best level, and its
        records and stored header carry that level (serialise it with with_zero_lf_deltas( ext ) and the level in the header).
        Synchronous."""
        import torch
        n = len(decoders)
        if len(frame_indices) != n or len(originals) != n:
            raise ValueError("lf_search_decode: need as many frame indices and originals as decoders")
        if measure not in self.LF_MEASURES:
            raise ValueError("lf_search_decode: measure is \"ssim\" or \"sse\", not %r" % (measure,))
        los = list(level_lo) if isinstance(level_lo, (list, tuple)) else [level_lo] * n
        his = list(level_hi) if isinstance(level_hi, (list, tuple)) else [level_hi] * n
        if len(los) != n or len(his) != n:
            raise ValueError("lf_search_decode: level_lo / level_hi are one for all jobs or one per job")
        jobs = (capi.LfSearchJob * max(n, 1))()
        keep = []
        for i, (d, t) in enumerate(zip(decoders, originals)):
            t = self._target_planes("lf_search_decode", i, d, t)
            j = jobs[i]
            j.stream, j.frame_index, j.level_lo, j.level_hi = d.h, int(frame_indices[i]), int(los[i]), int(his[i])
            j.original.y, j.original.u, j.original.v = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
            j.original.y_stride, j.original.uv_stride = t[0].stride(0), t[1].stride(0)
            keep.append(t)
        if n:
            torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()      # (the originals are ready; the call itself waits for its kernels)
        capi.check(self.L.aa_lf_search_decode_batch(self.h, jobs, n, self.LF_MEASURES[measure]))
        return [(jobs[i].best_level, jobs[i].best_score, jobs[i].evaluated) for i in range(n)]

    def set_lf_search_round(self, levels, jobs_per_slice=0):
        """Levels per job and round of lf_search_decode (1..8, default 4) and jobs per slice (0: by memory) -- aa_ctx_set_lf_search_round."""
        capi.check(self.L.aa_ctx_set_lf_search_round(self.h, int(levels), int(jobs_per_slice)))

    def lf_search_timing(self):
        """The last lf_search_decode of this context (aa_lf_search_last_timing), ms: the call (wall clock), then by HIP events the
        unfiltered reconstruction, k_lf_candidates, the candidates' loop filter, the scoring, k_lf_choose with the states coming down,
        k_lf_finish with the final filter; and the number of rounds."""
        out = (C.c_double * 8)()
        capi.check(self.L.aa_lf_search_last_timing(self.h, out))
        return dict(zip(("call_ms", "reconstruct_ms", "candidates_ms", "filter_ms", "score_ms", "choose_ms", "finish_ms", "rounds"), out))

    def _hash_streams(self, what, decoders):
        n = len(decoders)
        if n == 0:
            raise ValueError("%s: need at least one decoder" % what)
        for i, d in enumerate(decoders):
            if d.ctx is not self:
                raise ValueError("%s: decoders[%d] is a decoder of another context" % (what, i))
        return n, (C.c_void_p * n)(*[d.h for d in decoders])

    def raster_hashes(self, decoders, frame_indices, wait=True):
        """BaseRaster::raw_hash of frame frame_indices[i] of decoders[i] (aa_hash_rasters_async): what Decoder.raster_hash gives, for
        all of them by one kernel -- a GPU lane per raster -- without a download.  -> [int]; wait=False: a HashResult whose .result()
        waits.  The frames may be released right after the call."""
        n, arr = self._hash_streams("raster_hashes", decoders)
        if len(frame_indices) != n:
            raise ValueError("raster_hashes: need as many frame indices as decoders")
        out = (C.c_uint64 * n)()
        capi.check(self.L.aa_hash_rasters_async(self.h, arr, n, (C.c_int * n)(*frame_indices), out))
        r = HashResult(self, (out,), lambda: list(out))
        return r.result() if wait else r

    def decoder_hashes(self, decoders, wait=True):
        """DecoderHash of every decoder (aa_hash_decoders_async) -> [([state, last, golden, alternative], hash of the four)], what
        Decoder.decoder_hash gives; afterwards decoder_hash / minihash / raster_hash of these decoders answer from the cache."""
        n, arr = self._hash_streams("decoder_hashes", decoders)
        parts, whole = (C.c_uint64 * (4 * n))(), (C.c_uint64 * n)()
        capi.check(self.L.aa_hash_decoders_async(self.h, arr, n, parts, whole, None))
        r = HashResult(self, (parts, whole), lambda: [(list(parts[4 * i:4 * i + 4]), whole[i]) for i in range(n)])
        return r.result() if wait else r

    def minihashes(self, decoders, wait=True):
        """Decoder::minihash of every decoder (the low 32 bits of the DecoderHash's hash) -> [int]."""
        n, arr = self._hash_streams("minihashes", decoders)
        mini = (C.c_uint32 * n)()
        capi.check(self.L.aa_hash_decoders_async(self.h, arr, n, None, None, mini))
        r = HashResult(self, (mini,), lambda: list(mini))
        return r.result() if wait else r

    def hash_wait(self):
        """aa_ctx_hash_wait: every outstanding hash call is committed (arrays written, raster caches filled, rasters let go)."""
        try:
            capi.check(self.L.aa_ctx_hash_wait(self.h))
        finally:
            del self._hash_keep[:]

    def hash_stats(self, reset=False):
        """-> {"chains", "bytes", "cache_hits", "cache_fills"}: chains launched, bytes walked, rasters answered from the cache, cache
        entries filled (aa_ctx_hash_stats)."""
        out = (C.c_uint64 * 4)()
        capi.check(self.L.aa_ctx_hash_stats(self.h, out, int(reset)))
        return dict(zip(("chains", "bytes", "cache_hits", "cache_fills"), out))

    def hash_stream(self):
        return self.L.aa_ctx_hash_stream(self.h)

    def decode_batch(self, decoders, frame_indices):
        n = len(decoders)
        arr = (C.c_void_p * n)(*[d.h for d in decoders])
        idx = (C.c_int * n)(*frame_indices)
        capi.check(self.L.aa_decode_batch(self.h, arr, n, idx))


class HashResult:
    """An outstanding hash call (Context.raster_hashes / decoder_hashes / minihashes with wait=False): result() waits (for every
    outstanding call of the context) and returns the values."""

    def __init__(self, ctx, arrays, read):
        self.ctx, self._read, self._value = ctx, read, None
        ctx._hash_keep.append(arrays)        # (the runtime writes into them at the wait: the context holds them until then)

    def result(self):
        if self._read is not None:
            self.ctx.hash_wait()
            self._value, self._read = self._read(), None
        return self._value


class Decoder:
    """Decoder(width, height) of the reference, rasters resident in HBM."""

    def __init__(self, ctx, width, height):
        self.ctx, self.L = ctx, capi.lib()
        self.h = C.c_void_p()
        capi.check(self.L.aa_stream_create(ctx.h, width, height, C.byref(self.h)))
        self.width, self.height = width, height
        self.padded_width, self.padded_height = capi.raster_geometry(width, height)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.aa_stream_destroy(self.h); self.h = None

    def set_error_concealment(self, on):
        """Decoder::set_error_concealment (decoder.hh:298): accept frames that end early (host and GPU parser alike)."""
        capi.check(self.L.aa_stream_set_error_concealment(self.h, int(on)))

    def error_concealment(self):
        return bool(self.L.aa_stream_error_concealment(self.h))

    # -- two-step form: parse_frame + decode_frame (decoder.cc:89-118) --
    def parse_frame(self, frame_bytes):
        fi, hdr = C.c_int(), FrameHeader()
        capi.check(self.L.aa_stream_parse(self.h, frame_bytes, len(frame_bytes), C.byref(fi), C.byref(hdr)))
        return fi.value, hdr.as_dict()

    def append_records(self, header, mb, coeff_blocks):
        """A frame given as records (aa_stream_append_records): header dict as frame_header() / Parser.parse() return it,
        macroblock records, coefficient blocks [n, 16] -> frame index.  What an encoder has in hand when it updates its
        references (Encoder::write_frame, encoder.cc:146-160)."""
        hdr = FrameHeader()
        for n, _ in FrameHeader._fields_:
            if n == "quant":
                for sgm in range(4):
                    for k in range(6):
                        hdr.quant[sgm][k] = header["quant"][sgm][k]
            else:
                setattr(hdr, n, header[n])
        mbs = np.ascontiguousarray(mb, dtype=MB_INFO_DTYPE).reshape(-1)
        cf = np.ascontiguousarray(coeff_blocks, dtype=np.int16).reshape(-1, 16)
        hdr.num_coeff_blocks = len(cf)
        fi = C.c_int()
        capi.check(self.L.aa_stream_append_records(self.h, C.byref(hdr), mbs.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), C.byref(fi)))
        return fi.value

    def rebase(self, header, mb, target, records=True):
        """One new frame of this decoder by rebase (Context.rebase) -> (frame_index, mb [mbh, mbw], coeff_blocks [n, 16]), or with
        records=False (frame_index, num_coeff_blocks) and the records left on the device."""
        return self.ctx.rebase([self], [header], [mb], [target], records=records)[0]

    def reencode_as_inter(self, header, target, quality="best", append=True, records=True):
        """One new frame of this decoder by re-encode (Context.reencode_as_inter) -> (frame_index, mb [mbh, mbw], coeff_blocks [n, 16]), or
        with records=False (frame_index, num_coeff_blocks)."""
        return self.ctx.reencode_as_inter([self], [header], [target], quality, append, records)[0]

    def encode_frame(self, header, target, quality="best", append=True, records=True, two_pass=False):
        """One new frame of this decoder by the forward encoder (Context.encode_frames), a key frame where header["key_frame"] is set ->
        (frame_index, mb [mbh, mbw], coeff_blocks [n, 16]), or with records=False (frame_index, num_coeff_blocks); with two_pass (a key
        frame in the reference's two passes) one more element, the first pass's token_prob_update."""
        return self.ctx.encode_frames([self], [header], [target], quality, append, records, two_pass)[0]

    def estimate_frame_size(self, target, q_index, key_frame=False, quality="best", carry=None):
        """The frame-size estimate of one picture against this decoder (Context.estimate_frame_sizes) -> (size, carry after)."""
        return self.ctx.estimate_frame_sizes([self], [target], [q_index], key_frame, quality, None if carry is None else [carry])[0]

    def target_size_q(self, target, target_size, q_lo=4, q_hi=127, key_frame=False, quality="best", carry=None):
        """The quantiser index for a target frame size of one picture against this decoder (Context.target_size_q) -> (q_index, [(q, size)]
        visited, carry after)."""
        return self.ctx.target_size_q([self], [target], [target_size], q_lo, q_hi, key_frame, quality, None if carry is None else [carry])[0]

    def serialize_frame(self, frame_index, header, ext, probs_before=None, advance_state=False, capacity=None, sub_modes=None, optimise=False, details=False,
                        first_pass_updates=None):
        """One frame of this decoder, held as records, as VP8 bytes (Context.serialize_frames)."""
        return self.ctx.serialize_frames([self], [frame_index], [header], [ext], None if probs_before is None else [probs_before], advance_state, capacity,
                                         optimise=optimise, sub_modes=None if sub_modes is None else [sub_modes], details=details,
                                         first_pass_updates=None if first_pass_updates is None else [first_pass_updates])[0]

    def header_ext(self):
        """Parser.header_ext for this decoder's own parser: the frame parse_frame / get_frame_output / submit_frames parsed last."""
        x = capi.FrameHeaderExt()
        capi.check(self.L.aa_stream_last_header_ext(self.h, C.byref(x)))
        return x.as_dict()

    def upload(self):
        capi.check(self.L.aa_stream_upload(self.h))

    def release_staging(self):
        """Free the pinned host staging of everything parsed so far (uploads it first)."""
        capi.check(self.L.aa_stream_release_staging(self.h))

    def decode_frame(self, frame_index):
        self.ctx.decode_batch([self], [frame_index])

    # -- one-step form: get_frame_output (decoder.cc:125-135) -> (shown, frame index of the raster) --
    def get_frame_output(self, frame_bytes):
        fi, shown = C.c_int(), C.c_int()
        capi.check(self.L.aa_stream_decode(self.h, frame_bytes, len(frame_bytes), C.byref(fi), C.byref(shown)))
        return bool(shown.value), fi.value

    def parse_and_decode_frame(self, frame_bytes):
        shown, fi = self.get_frame_output(frame_bytes)
        return fi if shown else None

    def frame_count(self):
        return self.L.aa_stream_frame_count(self.h)

    def frame_header(self, frame_index):
        hdr = FrameHeader()
        capi.check(self.L.aa_stream_frame_header(self.h, frame_index, C.byref(hdr)))
        return hdr.as_dict()

    def read_records(self, frame_index):
        """A frame's parsed records as they sit in HBM -> (header dict, mb_info [mbh, mbw], coefficient blocks [n, 16])."""
        h = self.frame_header(frame_index)
        mbw, mbh = h["mb_width"], h["mb_height"]
        mb = np.zeros(mbw * mbh, dtype=MB_INFO_DTYPE)
        cf = np.zeros((max(1, h["num_coeff_blocks"]), 16), dtype=np.int16)
        capi.check(self.L.aa_stream_read_records(self.h, frame_index, mb.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), len(cf)))
        return h, mb.reshape(mbh, mbw), cf[:h["num_coeff_blocks"]]

    def rewind(self):
        capi.check(self.L.aa_stream_rewind(self.h))

    def decoder_hash(self):
        """DecoderHash (decoder.cc:143-153): ([state, last, golden, alternative], hash of the four)."""
        parts, whole = (C.c_uint64 * 4)(), C.c_uint64()
        capi.check(self.L.aa_stream_decoder_hash(self.h, parts, C.byref(whole)))
        return list(parts), whole.value

    def minihash(self):
        h = C.c_uint32()
        capi.check(self.L.aa_stream_minihash(self.h, C.byref(h)))
        return h.value

    def raster_hash(self, frame_index):
        h = C.c_uint64()
        capi.check(self.L.aa_stream_raster_hash(self.h, frame_index, C.byref(h)))
        return h.value

    def release_frame(self, frame_index):
        capi.check(self.L.aa_stream_release_frame(self.h, frame_index))

    def rewind_to(self, frame_index):
        capi.check(self.L.aa_stream_rewind_to(self.h, frame_index))

    def lf_search(self, frame_bytes, original_luma, level_lo, level_hi, want_rasters=False):
        """Encoder::apply_best_loopfilter_settings (encoder.cc:459-516) as one batch: -> (best level, its SSIM, [SSIM of every
        candidate], [raster bytes of every candidate] or None).  original_luma: padded_height x padded_width uint8."""
        n = level_hi - level_lo + 1
        orig = np.ascontiguousarray(original_luma, dtype=np.uint8)
        assert orig.shape == (self.padded_height, self.padded_width), orig.shape
        best, q = C.c_int(), C.c_double()
        qs = (C.c_double * n)()
        rb = sum(self.plane_sizes())
        rasters = np.empty(n * rb, np.uint8) if want_rasters else None
        capi.check(self.L.aa_stream_lf_search(self.h, frame_bytes, len(frame_bytes), orig.ctypes.data_as(C.c_void_p), level_lo, level_hi,
                                              C.byref(best), C.byref(q), qs, rasters.ctypes.data_as(C.c_void_p) if want_rasters else None))
        return best.value, q.value, list(qs), ([rasters[i * rb:(i + 1) * rb].tobytes() for i in range(n)] if want_rasters else None)

    def lf_search_decode(self, frame_index, original, level_lo=0, level_hi=63, measure="ssim"):
        """This decoder's next frame searched for its loop-filter level and decoded (Context.lf_search_decode)
        -> (best_level, best_score, evaluated)."""
        return self.ctx.lf_search_decode([self], [frame_index], [original], level_lo, level_hi, measure)[0]

    def release_before(self, first_kept):
        capi.check(self.L.aa_stream_release_before(self.h, first_kept))

    def raster(self, frame_index):
        """VP8Raster of a decoded frame as three padded numpy planes (lazy D2H, like RasterHandle::get())."""
        pw, ph = self.padded_width, self.padded_height
        y = np.empty((ph, pw), np.uint8); u = np.empty((ph // 2, pw // 2), np.uint8); v = np.empty((ph // 2, pw // 2), np.uint8)
        capi.check(self.L.aa_stream_download(self.h, frame_index, y.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)))
        return y, u, v

    def download_async(self, frame_index, y_ptr, u_ptr, v_ptr):
        """aa_stream_download_async: the frame's planes into PINNED host memory (Context.pinned_alloc), queued on the copy stream
        behind what the compute stream holds now; valid after Context.download_wait()."""
        capi.check(self.L.aa_stream_download_async(self.h, frame_index, C.c_void_p(y_ptr), C.c_void_p(u_ptr), C.c_void_p(v_ptr)))

    def download_wait(self):
        capi.check(self.L.aa_stream_download_wait(self.h))

    def raster_bytes(self, frame_index):
        return b"".join(p.tobytes() for p in self.raster(frame_index))

    def display_bytes(self, frame_index):
        """BaseRaster::dump (raster.cc:85-114): display rectangle as planar I420."""
        y, u, v = self.raster(frame_index)
        w, h = self.width, self.height
        return y[:h, :w].tobytes() + u[:(h + 1) // 2, :(w + 1) // 2].tobytes() + v[:(h + 1) // 2, :(w + 1) // 2].tobytes()

    def rgb(self, frame_index, format="rgb24", mean=None, std=None, out=None):
        """One frame as RGB on the device (Context.to_rgb): (H, W, 3|4) or (3, H, W); out: a tensor of that shape."""
        return self.ctx.to_rgb([self], [frame_index], format, mean, std, None if out is None else [out])[0]

    def quality(self, frame_index, original, planes="y"):
        """One frame against its original on the device (Context.quality) -> Quality(ssim (P,), sse (P,))."""
        q = self.ctx.quality([self], [frame_index], [original], planes)
        return Quality(q.ssim[0], q.sse[0])

    def raster_device_pointers(self, frame_index):
        y, u, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        capi.check(self.L.aa_stream_raster_device(self.h, frame_index, C.byref(y), C.byref(u), C.byref(v)))
        return y.value, u.value, v.value

    def get_references(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        capi.check(self.L.aa_stream_references(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"last": a.value, "golden": b.value, "alternative": c.value}

    def export_state(self):
        n = self.L.aa_stream_state_size(self.h)
        buf = (C.c_uint8 * n)()
        capi.check(self.L.aa_stream_export_state(self.h, buf, n))
        return bytes(buf)

    def import_state(self, blob):
        capi.check(self.L.aa_stream_import_state(self.h, blob, len(blob)))

    def serialize(self):
        """The decoder as the reference writes it to a .state file (Decoder::serialize, decoder.cc:54-69)."""
        n = C.c_size_t(0)
        capi.check(self.L.aa_stream_serialize(self.h, None, 0, C.byref(n)))
        buf = (C.c_uint8 * n.value)()
        capi.check(self.L.aa_stream_serialize(self.h, buf, n.value, C.byref(n)))
        return bytes(buf)

    def deserialize(self, blob):
        """Load a reference-format decoder state (EncoderStateDeserializer::build<Decoder>, decoder.cc:48-52,71-81)."""
        capi.check(self.L.aa_stream_deserialize(self.h, blob, len(blob)))

    def plane_sizes(self):
        pw, ph = self.padded_width, self.padded_height
        return pw * ph, (pw // 2) * (ph // 2), (pw // 2) * (ph // 2)

    def export_raster_device(self, frame_index, y_ptr, u_ptr, v_ptr):
        """D2D copy of a decoded raster into caller-owned device planes (async on the compute stream)."""
        capi.check(self.L.aa_stream_export_raster(self.h, frame_index, C.c_void_p(y_ptr), C.c_void_p(u_ptr), C.c_void_p(v_ptr)))

    def import_reference_device(self, y_ptr, u_ptr, v_ptr):
        capi.check(self.L.aa_stream_import_reference(self.h, C.c_void_p(y_ptr), C.c_void_p(u_ptr), C.c_void_p(v_ptr)))

    def import_reference_host(self, y, u, v):
        y, u, v = (np.ascontiguousarray(p, dtype=np.uint8) for p in (y, u, v))
        capi.check(self.L.aa_stream_import_reference_host(self.h, y.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)))


def with_zero_lf_deltas(ext):
    """A header extension (dict, as Parser.header_ext returns it) that writes the loop-filter adjustments as the reference's encoder
    leaves them after its level search (encoder.cc:464-470): lf_delta_update 1, every reference and mode delta present and zero.  What a
    frame searched by lf_search_decode is serialised with -- together with filter_adjustments_enabled = 1 and the chosen level in the
    header; the decoder that parses those bytes then filters with the level alone.  -> a new dict."""
    out = dict(ext)
    out["lf_delta_update"] = 1
    out["ref_lf_update"], out["mode_lf_update"] = [1] * 4, [1] * 4
    out["ref_lf_delta"], out["mode_lf_delta"] = [0] * 4, [0] * 4
    return out


def psnr(sse, width, height, planes):
    """10 log10(255^2 pixels / sse) of Quality.sse (torch, (..., P)) for padded planes of width x height luma pixels: planes "y" or
    "yuv" (chroma planes hold a quarter of the pixels); inf where sse == 0."""
    import torch
    pixels = [float(width * height)] + [float((width // 2) * (height // 2))] * 2
    count = torch.tensor(pixels[:Context.QUALITY_PLANES[planes]], dtype=torch.float64, device=sse.device)
    s = sse.to(torch.float64)
    return torch.where(s == 0, torch.full_like(s, float("inf")), 10.0 * torch.log10(255.0 * 255.0 * count / s))


def read_ivf(path_or_bytes):
    """IVF container (util/ivf.cc:36-82): -> (width, height, [frame bytes])."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if data[:4] != b"DKIF":
        raise AlfalfaError(-1, "invalid bitstream: missing IVF file header")
    if struct.unpack_from("<H", data, 4)[0] != 0:
        raise AlfalfaError(-2, "unsupported bitstream: not an IVF version 0 file")
    hdr_len = struct.unpack_from("<H", data, 6)[0]
    if hdr_len != 32:
        raise AlfalfaError(-2, "unsupported bitstream: unsupported IVF header length")
    width, height = struct.unpack_from("<HH", data, 12)
    nframes = struct.unpack_from("<I", data, 24)[0]
    frames, pos = [], hdr_len
    for _ in range(nframes):
        if pos + 12 > len(data):
            raise AlfalfaError(-1, "invalid bitstream: IVF file truncated")
        n = struct.unpack_from("<I", data, pos)[0]
        if pos + 12 + n > len(data):
            raise AlfalfaError(-1, "invalid bitstream: IVF file truncated")
        frames.append(bytes(data[pos + 12:pos + 12 + n])); pos += 12 + n
    return width, height, frames


class FilePlayer:
    """FilePlayer (player.cc:85-144): starts at the first key frame; advance() returns the next SHOWN raster."""

    def __init__(self, ctx, path_or_bytes):
        self.width, self.height, self.frames = read_ivf(path_or_bytes)
        self.decoder = Decoder(ctx, self.width, self.height)
        self.frame_no = 0
        while self.frame_no < len(self.frames) and (self.frames[self.frame_no][0] & 1):
            self.frame_no += 1

    def eof(self):
        return self.frame_no == len(self.frames)

    def advance(self):
        while not self.eof():
            fi = self.decoder.parse_and_decode_frame(self.frames[self.frame_no]); self.frame_no += 1
            if fi is not None:
                return fi
        raise AlfalfaError(-2, "unsupported bitstream: hidden frames at end of file")
