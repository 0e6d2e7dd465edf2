"""Decoded frames to RGB on the GPU (aa_render_rgb_async / Context.to_rgb): every case equals the numpy restatement of the
conversion (tests/rgb_reference.py) bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import alfalfa_amd as aa
from alfalfa_amd import capi
import rgb_reference as rr
from conftest import GOLDEN, GOLDEN_DIR

pytestmark = pytest.mark.gpu

CHW_DTYPES = {"chw_u8": torch.uint8, "chw_f16": torch.float16, "chw_bf16": torch.bfloat16, "chw_f32": torch.float32}


def host_bits(t):
    """A rendered tensor on the host, float formats as bit patterns (what rr.expected returns)."""
    t = t.cpu()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return rr.as_bits(t.numpy())


def decode_all(ctx, name):
    """-> decoder and the frame indices of its shown frames (all held)."""
    w, h, frames = aa.read_ivf(os.path.join(GOLDEN_DIR, name + ".ivf"))
    d = aa.Decoder(ctx, w, h)
    shown = []
    for fr in frames:
        s, fi = d.get_frame_output(fr)
        if s:
            shown.append(fi)
    return d, shown


@pytest.mark.parametrize("fmt", rr.FORMATS)
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_every_shown_golden_frame_in_every_format(gpu_ctx, name, fmt):
    d, shown = decode_all(gpu_ctx, name)
    out = gpu_ctx.to_rgb([d] * len(shown), shown, format=fmt)
    torch.cuda.synchronize()
    for i, fi in enumerate(shown):
        want = rr.expected(d.raster(fi), d.width, d.height, fmt)
        got = host_bits(out[i])
        assert got.shape == want.shape and np.array_equal(got, want), "%s frame %d" % (name, fi)
    one = d.rgb(shown[-1], format=fmt)
    assert np.array_equal(host_bits(one), rr.expected(d.raster(shown[-1]), d.width, d.height, fmt))


@pytest.mark.parametrize("fmt", ["rgb24", "chw_f32"])
def test_one_call_mixes_every_golden_size(gpu_ctx, fmt):
    decs = [decode_all(gpu_ctx, name) for name in sorted(GOLDEN)]
    ds, fis = [d for d, s in decs], [s[-1] for d, s in decs]
    with pytest.raises(ValueError):
        gpu_ctx.to_rgb(ds, fis, format=fmt)
    dtype = torch.uint8 if fmt == "rgb24" else torch.float32
    outs = [torch.empty((d.height, d.width, 3) if fmt == "rgb24" else (3, d.height, d.width), dtype=dtype, device="cuda") for d in ds]
    res = gpu_ctx.to_rgb(ds, fis, format=fmt, out=outs)
    assert res is not None and len(res) == len(ds)
    for d, fi, t in zip(ds, fis, outs):
        assert np.array_equal(host_bits(t), rr.expected(d.raster(fi), d.width, d.height, fmt))


@functools.lru_cache(maxsize=1)
def synth_1080p():
    import vp8_synth
    return [vp8_synth.perf_stream(1920, 1080, 9100 + s, 2).frames for s in range(8)]


@pytest.mark.parametrize("fmt", ["rgb24", "chw_bf16"])
def test_batch_of_32_synthetic_1080p_streams_in_one_call(gpu_ctx, fmt):
    streams = synth_1080p()
    ds, fis = [], []
    for i in range(32):
        d = aa.Decoder(gpu_ctx, 1920, 1080)
        idx = [d.get_frame_output(fr)[1] for fr in streams[i % 8]]
        ds.append(d); fis.append(idx[i % 2])
    out = gpu_ctx.to_rgb(ds, fis, format=fmt)
    assert tuple(out.shape) == ((32, 1080, 1920, 3) if fmt == "rgb24" else (32, 3, 1080, 1920))
    for i in range(32):
        assert np.array_equal(host_bits(out[i]), rr.expected(ds[i].raster(fis[i]), 1920, 1080, fmt)), "stream %d" % i


def _canary_views(n, shape_of, fmt, pad_elems, byte_offset):
    """A canary-filled byte buffer and a strided view into it of the frames' shape with padded rows (and planes)."""
    dtype = torch.uint8 if fmt in ("rgb24", "rgba", "chw_u8") else CHW_DTYPES[fmt]
    es = torch.tensor([], dtype=dtype).element_size()
    frame = shape_of
    if fmt in ("rgb24", "rgba"):
        h, w, c = frame
        rs = w * c + pad_elems
        fs = h * rs + 7
        strides = (fs, rs, c, 1)
    else:
        _, h, w = frame
        rs = w + pad_elems
        ps = h * rs + 5
        fs = 3 * ps + 3
        strides = (fs, ps, rs, 1)
    off = byte_offset // es
    total = off + n * fs + 64
    buf8 = torch.full((total * es,), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf8.view(dtype).as_strided((n,) + tuple(frame), strides, off)
    mask = torch.zeros(total, dtype=torch.bool)
    mask.as_strided((n,) + tuple(frame), strides, off).fill_(True)
    return buf8, view, mask.repeat_interleave(es).numpy()


@pytest.mark.parametrize("fmt", rr.FORMATS)
@pytest.mark.parametrize("name", ["synth_33x17_s7", "synth_175x143_s3", "qcif_q30"])
def test_out_views_with_padded_strides_leave_the_canaries(gpu_ctx, name, fmt):
    d, shown = decode_all(gpu_ctx, name)
    shape = (d.height, d.width, 4 if fmt == "rgba" else 3) if fmt in ("rgb24", "rgba") else (3, d.height, d.width)
    byte_offset = 1 if fmt in ("rgb24", "rgba", "chw_u8") else 0       # (float tensors are element-aligned)
    for pad in (3, 16):
        buf8, view, mask = _canary_views(len(shown), shape, fmt, pad, byte_offset)
        res = gpu_ctx.to_rgb([d] * len(shown), shown, format=fmt, out=view)
        assert res is view
        for i, fi in enumerate(shown):
            assert np.array_equal(host_bits(view[i]), rr.expected(d.raster(fi), d.width, d.height, fmt)), "frame %d" % fi
        raw = buf8.cpu().numpy()
        assert np.all(raw[~mask] == 0xA5), "bytes outside the rows were written"


@pytest.mark.parametrize("fmt", ["chw_f16", "chw_bf16", "chw_f32"])
def test_mean_and_std_on_float_formats(gpu_ctx, fmt):
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    d, shown = decode_all(gpu_ctx, "qvga_q100")
    out = gpu_ctx.to_rgb([d] * len(shown), shown, format=fmt, mean=mean, std=std)
    for i, fi in enumerate(shown):
        assert np.array_equal(host_bits(out[i]), rr.expected(d.raster(fi), d.width, d.height, fmt, mean, std))
    half = d.rgb(shown[0], format=fmt, mean=(0.5, 0.5, 0.5))
    assert np.array_equal(host_bits(half), rr.expected(d.raster(shown[0]), d.width, d.height, fmt, (0.5, 0.5, 0.5)))


def test_torch_reduction_on_the_current_stream_needs_no_sync(gpu_ctx):
    d, shown = decode_all(gpu_ctx, "cif_q60_lf40s5")
    want = [int(rr.expected(d.raster(fi), d.width, d.height, "rgb24").astype(np.int64).sum()) for fi in shown]
    got = [int(d.rgb(fi).to(torch.int64).sum().item()) for fi in shown]          # default (null) stream
    assert got == want
    want = [rr.expected(d.raster(fi), d.width, d.height, "chw_f32").view(np.float32).astype(np.float64).sum() for fi in shown]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sums = [d.rgb(fi, format="chw_f32").double().sum() for fi in shown]       # a stream of torch's own
        got = [x.item() for x in sums]
    assert np.allclose(got, want, rtol=1e-12, atol=0)


def test_render_then_release_then_decode_more_of_the_same_decoder(gpu_ctx):
    name = "s64_q5_rt"
    w, h, frames = aa.read_ivf(os.path.join(GOLDEN_DIR, name + ".ivf"))
    ref = aa.Decoder(gpu_ctx, w, h)
    want = []
    for fr in frames:
        s, fi = ref.get_frame_output(fr)
        if s:
            want.append(rr.expected(ref.raster(fi), w, h, "rgb24"))
    d = aa.Decoder(gpu_ctx, w, h)
    got = []
    for fr in frames:
        s, fi = d.get_frame_output(fr)
        if s:
            got.append(d.rgb(fi))
        d.release_frame(fi)                  # the raster may be recycled by the next decode: the render is ahead of it
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (g, wnt) in enumerate(zip(got, want)):
        assert np.array_equal(g.cpu().numpy(), wnt), "shown frame %d" % i


def test_rendering_changes_no_hash(gpu_ctx):
    d, shown = decode_all(gpu_ctx, "w200_q40_lf63s7")
    before = [d.raster_hash(fi) for fi in shown], d.decoder_hash()
    for fmt in rr.FORMATS:
        gpu_ctx.to_rgb([d] * len(shown), shown, format=fmt)
    torch.cuda.synchronize()
    assert ([d.raster_hash(fi) for fi in shown], d.decoder_hash()) == before


def _render(ctx, decs, fis, fmt, targets, mean=None, std=None, consumer=None):
    n = len(decs)
    arr = (C.c_void_p * n)(*[x.h for x in decs])
    idx = (C.c_int * n)(*fis)
    tg = (capi.RgbTarget * n)(*targets)
    m = None if mean is None else (C.c_double * 3)(*mean)
    sd = None if std is None else (C.c_double * 3)(*std)
    return capi.lib().aa_render_rgb_async(ctx.h, arr, n, idx, fmt, tg, m, sd, consumer)


def test_every_error_row_returns_its_status_with_a_message(gpu_ctx):
    L = capi.lib()
    d, shown = decode_all(gpu_ctx, "synth_33x17_s7")
    fi = shown[0]
    buf = torch.zeros(64 * 1024, dtype=torch.uint8, device="cuda")
    ok = capi.RgbTarget(buf.data_ptr(), 33 * 3, 0)
    chw = capi.RgbTarget(buf.data_ptr(), 33 * 4, 17 * 33 * 4)
    assert _render(gpu_ctx, [d], [fi], capi.AA_RGB_U8_HWC3, [ok]) == 0
    gpu_ctx.sync()
    other_ctx = aa.Context(0)
    other = aa.Decoder(other_ctx, 33, 17)
    rows = [
        (capi.AA_RGB_U8_HWC3, [other], [0], [ok], None, None, -7),                        # another context's stream
        (capi.AA_RGB_U8_HWC3, [d], [len(shown) + 100], [ok], None, None, -7),             # bad frame index
        (capi.AA_RGB_U8_HWC3, [d], [-1], [ok], None, None, -7),
        (capi.AA_RGB_U8_HWC3, [d], [fi], [capi.RgbTarget(buf.data_ptr(), 33 * 3 - 1, 0)], None, None, -7),   # row stride
        (capi.AA_RGB_F32_CHW, [d], [fi], [capi.RgbTarget(buf.data_ptr(), 33 * 4, 17 * 33 * 4 - 1)], None, None, -7),   # plane stride
        (6, [d], [fi], [ok], None, None, -7),                                              # unknown format
        (-1, [d], [fi], [ok], None, None, -7),
        (capi.AA_RGB_U8_HWC3, [d], [fi], [capi.RgbTarget(None, 33 * 3, 0)], None, None, -7),   # null dst
        (capi.AA_RGB_U8_CHW, [d], [fi], [chw], (0.5, 0.5, 0.5), None, -7),               # mean/std with a u8 format
        (capi.AA_RGB_F32_CHW, [d], [fi], [chw], None, (1.0, 0.0, 1.0), -7),               # std 0
    ]
    for fmt, decs, fis, tg, mean, std, code in rows:
        assert _render(gpu_ctx, decs, fis, fmt, tg, mean, std) == code, (fmt, fis, code)
        assert L.aa_last_error().decode().startswith("aa_render_rgb_async")
    # a frame parsed and not decoded yet; a released frame
    w, h, frames = aa.read_ivf(os.path.join(GOLDEN_DIR, "synth_33x17_s7.ivf"))
    p = aa.Decoder(gpu_ctx, w, h)
    pfi, _ = p.parse_frame(frames[0])
    assert _render(gpu_ctx, [p], [pfi], capi.AA_RGB_U8_HWC3, [ok]) == -3
    assert b"not decoded" in L.aa_last_error()
    d.release_frame(fi)
    assert _render(gpu_ctx, [d], [fi], capi.AA_RGB_U8_HWC3, [ok]) == -3
    assert b"released" in L.aa_last_error()
    with pytest.raises(capi.AlfalfaError):
        d.rgb(fi)
    with pytest.raises(ValueError):
        d.rgb(shown[1], format="yuv")
