"""Decoded frames scored against originals on the GPU (aa_quality_batch_async / Context.quality): SSIM equals the oracle's
(vo.ssim_plane, to which aa_ssim_host is pinned by test_ssim_oracle.py) bit for bit, the squared error equals numpy's."""
import ctypes as C
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import alfalfa_amd as aa
from alfalfa_amd import capi
import vp8_oracle as vo
import test_gpu_rgb as rgbt
from conftest import GOLDEN, GOLDEN_DIR

pytestmark = pytest.mark.gpu

AMPLITUDES = (0, 3, 40)


def planes_of(d):
    pw, ph = d.padded_width, d.padded_height
    return [(pw, ph), (pw // 2, ph // 2), (pw // 2, ph // 2)]


def noisy(raster, amp, rng):
    """The raster's three planes plus integer noise in [-amp, amp], clipped to bytes."""
    out = []
    for p in raster:
        nz = rng.integers(-amp, amp + 1, size=p.shape) if amp else np.zeros(p.shape, np.int64)
        out.append(np.clip(p.astype(np.int64) + nz, 0, 255).astype(np.uint8))
    return out


def expected(raster, orig, nplanes):
    """-> ([ssim per plane], [sse per plane]) from the oracle and numpy."""
    ssim, sse = [], []
    for a, b in list(zip(raster, orig))[:nplanes]:
        h, w = a.shape
        ssim.append(vo.ssim_plane(a.tobytes(), b.tobytes(), w, h))
        diff = a.astype(np.int64) - b.astype(np.int64)
        sse.append(int((diff * diff).sum()))
    return ssim, sse


def on_device(planes):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes)


def check(q, want, what=""):
    ssim, sse = q.ssim.cpu().numpy(), q.sse.cpu().numpy()
    assert q.ssim.dtype == torch.float64 and q.sse.dtype == torch.int64
    for i, (ws, we) in enumerate(want):
        assert ssim[i].tolist() == ws, "%s pair %d: ssim %r, oracle %r" % (what, i, ssim[i].tolist(), ws)
        assert sse[i].tolist() == we, "%s pair %d: sse %r, numpy %r" % (what, i, sse[i].tolist(), we)


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """Host side of one golden stream, made once: per shown frame the oracle-side original (decoded + noise) and what to expect.
    The rasters come from the oracle decoder, which the GPU decode equals (test_gpu_parity.py)."""
    w, h, frames = vo.read_ivf(os.path.join(GOLDEN_DIR, name + ".ivf"))
    ora = vo.OracleDecoder(w, h)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cases = []
    for fr in frames:
        if not ora.decode(fr):
            continue
        y, u, v = ora.planes()
        amp = AMPLITUDES[len(cases) % 3]
        orig = noisy((y, u, v), amp, rng)
        cases.append((amp, orig, expected((y, u, v), orig, 3)))
    return cases


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_every_shown_golden_frame_yuv(gpu_ctx, name):
    d, shown = rgbt.decode_all(gpu_ctx, name)
    cases = golden_case(name)
    assert len(cases) == len(shown)
    q = gpu_ctx.quality([d] * len(shown), shown, [on_device(c[1]) for c in cases], planes="yuv")
    assert tuple(q.ssim.shape) == tuple(q.sse.shape) == (len(shown), 3)
    check(q, [c[2] for c in cases], name)
    for i, (amp, _, (ssim, sse)) in enumerate(cases):
        if amp == 0:
            assert sse == [0, 0, 0] and all(abs(s - 1.0) < 1e-6 for s in ssim)
            assert q.sse[i].tolist() == [0, 0, 0] and all(abs(s - 1.0) < 1e-6 for s in q.ssim[i].tolist())
    one = d.quality(shown[-1], on_device(cases[-1][1]), planes="yuv")
    assert one.ssim.tolist() == cases[-1][2][0] and one.sse.tolist() == cases[-1][2][1]


@pytest.mark.parametrize("planes", ["y", "yuv"])
def test_one_call_mixes_every_golden_size(gpu_ctx, planes):
    np_ = 1 if planes == "y" else 3
    decs = [rgbt.decode_all(gpu_ctx, name) for name in sorted(GOLDEN)]
    ds, fis, origs, want = [], [], [], []
    for name, (d, shown) in zip(sorted(GOLDEN), decs):
        k = 1 if len(shown) > 1 else 0                     # (a frame with noise: amplitude 3)
        amp, orig, (ssim, sse) = golden_case(name)[k]
        ds.append(d); fis.append(shown[k]); want.append((ssim[:np_], sse[:np_]))
        origs.append(on_device(orig) if planes == "yuv" else (on_device(orig[:1])[0], None, None))
    q = gpu_ctx.quality(ds, fis, origs, planes=planes)
    assert tuple(q.ssim.shape) == (len(ds), np_)
    check(q, want, planes)


def test_eight_1080p_decoders_yuv(gpu_ctx):
    streams = rgbt.synth_1080p()
    rng = np.random.default_rng(1080)
    ds, fis, origs, want = [], [], [], []
    for i in range(8):
        d = aa.Decoder(gpu_ctx, 1920, 1080)
        idx = [d.get_frame_output(fr)[1] for fr in streams[i]]
        raster = d.raster(idx[-1])
        orig = noisy(raster, AMPLITUDES[1 + i % 2], rng)
        ds.append(d); fis.append(idx[-1]); origs.append(on_device(orig)); want.append(expected(raster, orig, 3))
    q = gpu_ctx.quality(ds, fis, origs, planes="yuv")
    check(q, want, "1080p")


@pytest.mark.parametrize("width,height", [(1936, 40), (1968, 24)])
def test_planes_wider_than_one_column_chunk(gpu_ctx, width, height):
    """A workgroup of the first pass holds 480 windows of a row: a padded luma plane of 1936 has 483 (a second chunk of 3), one of
    1968 has 491; their chroma planes are a single chunk."""
    import vp8_synth
    frames = vp8_synth.perf_stream(width, height, 77, 2).frames
    d = aa.Decoder(gpu_ctx, width, height)
    fis = [d.get_frame_output(fr)[1] for fr in frames]
    rng = np.random.default_rng(width)
    rasters = [d.raster(fi) for fi in fis]
    origs = [noisy(r, amp, rng) for r, amp in zip(rasters, (3, 40))]
    q = gpu_ctx.quality([d] * len(fis), fis, [on_device(o) for o in origs], planes="yuv")
    check(q, [expected(r, o, 3) for r, o in zip(rasters, origs)], "%dx%d" % (width, height))


def test_decoded_against_decoded_is_the_oracle_and_symmetric(gpu_ctx):
    a, sa = rgbt.decode_all(gpu_ctx, "qcif_q30")
    b, sb = rgbt.decode_all(gpu_ctx, "qcif_q30_lf24")
    n = min(len(sa), len(sb))
    want = [expected(a.raster(sa[i]), b.raster(sb[i]), 3) for i in range(n)]
    ab = gpu_ctx.quality([a] * n, sa[:n], [(b, sb[i]) for i in range(n)], planes="yuv")
    ba = gpu_ctx.quality([b] * n, sb[:n], [(a, sa[i]) for i in range(n)], planes="yuv")
    check(ab, want, "a:b")
    assert torch.equal(ab.ssim, ba.ssim) and torch.equal(ab.sse, ba.sse)
    assert any(e != [0, 0, 0] for _, e in want)              # (the two streams do differ)


@pytest.mark.parametrize("name", ["synth_33x17_s7", "synth_175x143_s3", "qcif_q30"])
def test_originals_as_views_with_padded_rows(gpu_ctx, name):
    d, shown = rgbt.decode_all(gpu_ctx, name)
    cases = golden_case(name)
    views = []
    for _, orig, _ in cases:
        vs = []
        for p in orig:
            h, w = p.shape
            buf = torch.full((16 + h * (w + 48),), 0xA5, dtype=torch.uint8, device="cuda")
            view = buf.as_strided((h, w), (w + 48, 1), 16)
            view.copy_(torch.from_numpy(np.ascontiguousarray(p)))
            vs.append(view)
        views.append(tuple(vs))
    strided = gpu_ctx.quality([d] * len(shown), shown, views, planes="yuv")
    dense = gpu_ctx.quality([d] * len(shown), shown, [on_device(c[1]) for c in cases], planes="yuv")
    assert torch.equal(strided.ssim, dense.ssim) and torch.equal(strided.sse, dense.sse)
    check(strided, [c[2] for c in cases], name)


def test_torch_reduction_on_the_current_stream_needs_no_sync(gpu_ctx):
    name = "cif_q60_lf40s5"
    d, shown = rgbt.decode_all(gpu_ctx, name)
    cases = golden_case(name)
    origs = [on_device(c[1]) for c in cases]
    want_ssim = np.array([c[2][0] for c in cases]).sum()
    want_sse = sum(sum(c[2][1]) for c in cases)
    q = gpu_ctx.quality([d] * len(shown), shown, origs, planes="yuv")            # default (null) stream
    assert int(q.sse.sum().item()) == want_sse
    assert np.isclose(q.ssim.sum().item(), want_ssim, rtol=1e-12, atol=0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        q = gpu_ctx.quality([d] * len(shown), shown, origs, planes="yuv")        # a stream of torch's own
        got = q.ssim.sum(), q.sse.sum()
        assert int(got[1].item()) == want_sse
        assert np.isclose(got[0].item(), want_ssim, rtol=1e-12, atol=0)
    torch.cuda.current_stream().wait_stream(s)


def test_score_then_release_then_decode_more_of_the_same_decoder(gpu_ctx):
    name = "s64_q5_rt"
    w, h, frames = aa.read_ivf(os.path.join(GOLDEN_DIR, name + ".ivf"))
    cases = golden_case(name)
    origs = [on_device(c[1]) for c in cases]
    d = aa.Decoder(gpu_ctx, w, h)
    got = []
    for fr in frames:
        s, fi = d.get_frame_output(fr)
        if s:
            got.append(d.quality(fi, origs[len(got)], planes="yuv"))
        d.release_frame(fi)                  # the raster may be recycled by the next decode: the scoring is ahead of it
    torch.cuda.synchronize()
    assert len(got) == len(cases)
    for i, (g, c) in enumerate(zip(got, cases)):
        assert g.ssim.tolist() == c[2][0] and g.sse.tolist() == c[2][1], "shown frame %d" % i


def test_scoring_changes_no_hash(gpu_ctx):
    name = "w200_q40_lf63s7"
    d, shown = rgbt.decode_all(gpu_ctx, name)
    origs = [on_device(c[1]) for c in golden_case(name)]
    before = [d.raster_hash(fi) for fi in shown], d.decoder_hash()
    for planes in ("y", "yuv"):
        gpu_ctx.quality([d] * len(shown), shown, origs, planes=planes)
    gpu_ctx.quality([d] * len(shown), shown, [(d, fi) for fi in shown], planes="yuv")
    torch.cuda.synchronize()
    assert ([d.raster_hash(fi) for fi in shown], d.decoder_hash()) == before


def _score(ctx, decs, fis, refs, planes, ssim, sse, streams=True, indices=True, originals=True, n=None):
    k = len(decs)
    arr = (C.c_void_p * k)(*[x.h for x in decs]) if streams else None
    idx = (C.c_int * k)(*fis) if indices else None
    rf = (capi.QualityRef * k)(*refs) if originals else None
    return capi.lib().aa_quality_batch_async(ctx.h, arr, k if n is None else n, idx, rf, planes, ssim, sse, None)


def test_every_error_row_returns_its_status_with_a_message(gpu_ctx):
    L = capi.lib()
    name = "synth_33x17_s7"                                  # 48x32 padded luma, 24x16 chroma
    d, shown = rgbt.decode_all(gpu_ctx, name)
    fi = shown[0]
    case = golden_case(name)[0]
    y, u, v = on_device(case[1])
    ssim = torch.zeros(3, dtype=torch.float64, device="cuda")
    sse = torch.zeros(3, dtype=torch.int64, device="cuda")
    ok = capi.QualityRef(y.data_ptr(), u.data_ptr(), v.data_ptr(), 48, 24)
    sp, ep = C.c_void_p(ssim.data_ptr()), C.c_void_p(sse.data_ptr())

    def good():
        assert _score(gpu_ctx, [d], [fi], [ok], 3, sp, ep) == 0
        gpu_ctx.sync()
        assert ssim.tolist() == case[2][0] and sse.tolist() == case[2][1]

    good()
    other_ctx = aa.Context(0)
    other = aa.Decoder(other_ctx, 33, 17)
    rows = [
        (dict(streams=False), [d], [fi], [ok], 3, sp, -7),                                       # null arrays
        (dict(indices=False), [d], [fi], [ok], 3, sp, -7),
        (dict(originals=False), [d], [fi], [ok], 3, sp, -7),
        ({}, [d], [fi], [ok], 3, None, -7),                                                      # ... the result array too
        (dict(n=0), [d], [fi], [ok], 3, sp, -7),                                                 # n <= 0
        (dict(n=-1), [d], [fi], [ok], 3, sp, -7),
        ({}, [d], [fi], [ok], 2, sp, -7),                                                        # planes not 1 or 3
        ({}, [d], [fi], [ok], 0, sp, -7),
        ({}, [d], [fi], [capi.QualityRef(None, u.data_ptr(), v.data_ptr(), 48, 24)], 1, sp, -7),  # a null plane that is needed
        ({}, [d], [fi], [capi.QualityRef(y.data_ptr(), None, v.data_ptr(), 48, 24)], 3, sp, -7),
        ({}, [d], [fi], [capi.QualityRef(y.data_ptr(), u.data_ptr(), None, 48, 24)], 3, sp, -7),
        ({}, [d], [fi], [capi.QualityRef(y.data_ptr(), u.data_ptr(), v.data_ptr(), 47, 24)], 1, sp, -7),   # strides below the width
        ({}, [d], [fi], [capi.QualityRef(y.data_ptr(), u.data_ptr(), v.data_ptr(), 48, 23)], 3, sp, -7),
        ({}, [d], [d.frame_count() + 100], [ok], 3, sp, -7),                                     # frame index out of range
        ({}, [d], [-1], [ok], 3, sp, -7),
        ({}, [other], [0], [ok], 3, sp, -7),                                                     # another context's stream
    ]
    for kw, decs, fis, refs, planes, out, code in rows:
        assert _score(gpu_ctx, decs, fis, refs, planes, out, ep, **kw) == code, (kw, fis, planes, code)
        assert L.aa_last_error().decode().startswith("aa_quality_batch_async"), L.aa_last_error()
    # u and v are not looked at for Y alone
    assert _score(gpu_ctx, [d], [fi], [capi.QualityRef(y.data_ptr(), None, None, 48, 0)], 1, sp, None) == 0
    good()
    # a frame parsed and not decoded yet; a released frame
    w, h, frames = aa.read_ivf(os.path.join(GOLDEN_DIR, name + ".ivf"))
    p = aa.Decoder(gpu_ctx, w, h)
    pfi, _ = p.parse_frame(frames[0])
    assert _score(gpu_ctx, [p], [pfi], [ok], 3, sp, ep) == -3
    assert b"aa_quality_batch_async" in L.aa_last_error() and b"not decoded" in L.aa_last_error()
    good()
    d.release_frame(fi)
    assert _score(gpu_ctx, [d], [fi], [ok], 3, sp, ep) == -3
    assert b"aa_quality_batch_async" in L.aa_last_error() and b"released" in L.aa_last_error()
    with pytest.raises(capi.AlfalfaError):
        d.quality(fi, (y, u, v), planes="yuv")
    fi = shown[1]
    case = golden_case(name)[1]
    y, u, v = on_device(case[1])
    q = d.quality(fi, (y, u, v), planes="yuv")                                                   # a correct call still works
    assert q.ssim.tolist() == case[2][0] and q.sse.tolist() == case[2][1]
    # the Python layer names the offending entry
    bad = [
        ((y[:, :-1], u, v), "yuv"), ((y, u, None), "yuv"), ((y.to(torch.int8), u, v), "yuv"), ((y.cpu(), u, v), "yuv"),
        ((y.t().contiguous().t(), u, v), "yuv"), ((y, u), "yuv"), ((y, u, v), "uv"),
    ]
    for orig, planes in bad:
        with pytest.raises(ValueError) as e:
            gpu_ctx.quality([d, d], [fi, fi], [(y, u, v), orig], planes=planes)
        assert planes == "uv" or "originals[1]" in str(e.value), str(e.value)


def test_psnr_is_numpys_formula():
    sse = np.array([[0, 5, 123456], [98765432, 1, 0]], dtype=np.int64)
    w, h = 176, 144
    pixels = np.array([w * h, w * h // 4, w * h // 4], dtype=np.float64)
    with np.errstate(divide="ignore"):
        want = np.where(sse == 0, np.inf, 10.0 * np.log10(255.0 * 255.0 * pixels / sse.astype(np.float64)))
    got = aa.psnr(torch.from_numpy(sse).cuda(), w, h, "yuv").cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(np.isinf(got), sse == 0)
    assert np.allclose(got[sse != 0], want[sse != 0], rtol=1e-14, atol=0)
    got_y = aa.psnr(torch.from_numpy(sse[:, :1]).cuda(), w, h, "y").cpu().numpy()
    assert np.allclose(got_y[1:], want[1:, :1], rtol=1e-14, atol=0) and np.isinf(got_y[0, 0])
