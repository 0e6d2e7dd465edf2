"""The pinned job tables of the batched calls come from one ring type (16 entries per kind of call) and every call that reads a
decoded frame asks one question first.  Results only: rings that wrap with no sync in between, an entry that grows past its floor and
is used small again, and the status of every refused frame."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import alfalfa_amd as aa
from alfalfa_amd import capi
import rgb_reference as rr
import test_gpu_quality as qt
import test_gpu_rgb as rgbt
from conftest import GOLDEN, GOLDEN_DIR, golden_frames, sha256

pytestmark = pytest.mark.gpu

SMALL = "synth_33x17_s7"        # 33x17: 48x32 padded luma, 24x16 chroma
RING = 16                       # entries of a ring
BIG = 700                       # entries of a call above every floor (512 bindings / gather jobs / render jobs, 1536 scoring jobs = 512 x 3 planes)


def test_twenty_scoring_calls_without_a_sync(gpu_ctx):
    cases = qt.golden_case(SMALL)

    def calls(ctx, sync):
        d, shown = rgbt.decode_all(ctx, SMALL)
        origs = [qt.on_device(c[1]) for c in cases]
        out = []
        for k in range(20):
            pick = [(k + j) % len(shown) for j in range(1 + k % 3)]
            out.append((pick, ctx.quality([d] * len(pick), [shown[i] for i in pick], [origs[i] for i in pick], planes="yuv")))
            if sync:
                ctx.sync()
        return out

    fresh = aa.Context(0)
    want = [(pick, q.ssim.cpu(), q.sse.cpu()) for pick, q in calls(fresh, True)]
    got = calls(gpu_ctx, False)
    torch.cuda.synchronize()
    for k, ((pick, q), (_, ssim, sse)) in enumerate(zip(got, want)):
        assert torch.equal(q.ssim.cpu(), ssim) and torch.equal(q.sse.cpu(), sse), "call %d" % k
        qt.check(q, [cases[i][2] for i in pick], "call %d" % k)


def test_twenty_renders_without_a_sync(gpu_ctx):
    d, shown = rgbt.decode_all(gpu_ctx, SMALL)
    plan = [(shown[k % len(shown)], rr.FORMATS[k % len(rr.FORMATS)]) for k in range(20)]
    want = [rr.expected(d.raster(fi), d.width, d.height, fmt) for fi, fmt in plan]
    outs = [d.rgb(fi, format=fmt) for fi, fmt in plan]             # (20 tensors of their own)
    torch.cuda.synchronize()
    for k, (t, w) in enumerate(zip(outs, want)):
        assert np.array_equal(rgbt.host_bits(t), w), "call %d" % k


@pytest.mark.parametrize("call", ["rgb", "quality", "download"])
def test_an_entry_grows_and_is_used_small_again(gpu_ctx, call):
    """4 frames, 700 entries, 4 frames -- and the small call as often again as the ring has entries, so that the entry that grew
    comes round."""
    d, shown = rgbt.decode_all(gpu_ctx, SMALL)
    cases = qt.golden_case(SMALL)
    rasters = {fi: d.raster(fi) for fi in shown}
    sizes = [4, BIG, 4] + [4] * RING
    picks = [[(3 * k + j) % len(shown) for j in range(n)] for k, n in enumerate(sizes)]
    if call == "rgb":
        got = [gpu_ctx.to_rgb([d] * len(p), [shown[i] for i in p]) for p in picks]      # (a (n, 17, 33, 3) tensor: n targets)
        torch.cuda.synchronize()
        want = {i: rr.expected(rasters[shown[i]], d.width, d.height, "rgb24") for i in range(len(shown))}
        for k, (p, out) in enumerate(zip(picks, got)):
            host = out.cpu().numpy()
            for j, i in enumerate(p):
                assert np.array_equal(host[j], want[i]), "call %d entry %d" % (k, j)
    elif call == "quality":
        origs = [qt.on_device(c[1]) for c in cases]
        got = [gpu_ctx.quality([d] * len(p), [shown[i] for i in p], [origs[i] for i in p], planes="yuv") for p in picks]
        torch.cuda.synchronize()
        for k, (p, q) in enumerate(zip(picks, got)):
            qt.check(q, [cases[i][2] for i in p], "call %d" % k)
    else:
        stride = sum(d.plane_sizes())
        assert stride % 16 == 0
        slabs = [gpu_ctx.pinned_alloc(stride * len(p)) for p in picks]
        try:
            for p, slab in zip(picks, slabs):
                gpu_ctx.download_batch_async([d] * len(p), [shown[i] for i in p], slab, stride)
            gpu_ctx.download_wait()
            want = {i: b"".join(x.tobytes() for x in rasters[shown[i]]) for i in range(len(shown))}
            for k, (p, slab) in enumerate(zip(picks, slabs)):
                for j, i in enumerate(p):
                    assert C.string_at(slab + j * stride, stride) == want[i], "call %d entry %d" % (k, j)
        finally:
            gpu_ctx.sync()
            for slab in slabs:
                gpu_ctx.pinned_free(slab)


def test_twenty_two_decode_calls_without_a_sync(gpu_ctx):
    """No golden stream has 20 frames: two decoders take turns, one frame and one aa_decode_batch call at a time."""
    names = ["s64_q5_rt", SMALL]
    streams = [golden_frames(n) for n in names]
    decs = [aa.Decoder(gpu_ctx, w, h) for w, h, _ in streams]
    calls = 0
    for f in range(max(len(fr) for _, _, fr in streams)):
        for d, (_, _, frames) in zip(decs, streams):
            if f < len(frames):
                fi, _ = d.parse_frame(frames[f])
                gpu_ctx.decode_batch([d], [fi])
                calls += 1
    assert calls >= 20
    for d, n, (_, _, frames) in zip(decs, names, streams):
        for f in range(len(frames)):
            assert sha256(d.raster_bytes(f)) == GOLDEN[n]["raster_sha256"][f], (n, f)


def test_every_call_refuses_the_same_frames_with_the_same_status(gpu_ctx):
    L = capi.lib()
    w, h, frames = aa.read_ivf(os.path.join(GOLDEN_DIR, SMALL + ".ivf"))
    d, shown = rgbt.decode_all(gpu_ctx, SMALL)
    other_ctx = aa.Context(0)
    other = aa.Decoder(other_ctx, w, h)
    parsed = aa.Decoder(gpu_ctx, w, h)
    pfi, _ = parsed.parse_frame(frames[0])
    d.release_frame(shown[0])
    refused = [("another context's decoder", other, 0, -7), ("index -1", d, -1, -7), ("index past the end", d, d.frame_count() + 100, -7),
               ("parsed, not decoded", parsed, pfi, -3), ("released", d, shown[0], -3)]

    y, u, v = qt.on_device(qt.golden_case(SMALL)[0][1])
    ref = capi.QualityRef(y.data_ptr(), u.data_ptr(), v.data_ptr(), 48, 24)
    ssim = torch.zeros(3, dtype=torch.float64, device="cuda")
    sse = torch.zeros(3, dtype=torch.int64, device="cuda")
    rgb = torch.zeros((17, 33, 3), dtype=torch.uint8, device="cuda")
    target = capi.RgbTarget(rgb.data_ptr(), 33 * 3, 0)
    stride = sum(d.plane_sizes())
    slab = gpu_ctx.pinned_alloc(stride)
    hashes = (C.c_uint64 * 1)()

    def hash_rasters(dec, fi):
        return L.aa_hash_rasters_async(gpu_ctx.h, (C.c_void_p * 1)(dec.h), 1, (C.c_int * 1)(fi), hashes)

    def download(dec, fi):
        return L.aa_download_batch_async(gpu_ctx.h, (C.c_void_p * 1)(dec.h), 1, (C.c_int * 1)(fi), C.c_void_p(slab), stride)

    batched = {
        "aa_hash_rasters_async": hash_rasters,
        "aa_render_rgb_async": lambda dec, fi: rgbt._render(gpu_ctx, [dec], [fi], capi.AA_RGB_U8_HWC3, [target]),
        "aa_quality_batch_async": lambda dec, fi: qt._score(gpu_ctx, [dec], [fi], [ref], 3, C.c_void_p(ssim.data_ptr()), C.c_void_p(sse.data_ptr())),
        "aa_download_batch_async": download,
    }
    try:
        for name, call in batched.items():
            for what, dec, fi, status in refused:
                assert call(dec, fi) == status, (name, what)
                assert L.aa_last_error().decode().startswith(name + ":"), (name, what, L.aa_last_error())
        # Decoder.raster_hash names no context: a decoder is always its own context's
        for what, dec, fi, status in refused[1:]:
            assert L.aa_stream_raster_hash(dec.h, fi, hashes) == status, what
            assert L.aa_last_error().decode().startswith("aa_stream_raster_hash:"), (what, L.aa_last_error())
            with pytest.raises(capi.AlfalfaError):
                dec.raster_hash(fi)
        # ... and a frame that is held and decoded is served by all of them
        fi = shown[1]
        for name, call in batched.items():
            assert call(d, fi) == 0, name
        gpu_ctx.hash_wait()
        gpu_ctx.download_wait()
        gpu_ctx.sync()
        raster = d.raster(fi)
        twin, twin_shown = rgbt.decode_all(gpu_ctx, SMALL)           # (its raster_hash goes the per-stream route: no cache filled yet)
        assert hashes[0] == twin.raster_hash(twin_shown[1])
        assert np.array_equal(rgb.cpu().numpy(), rr.expected(raster, 33, 17, "rgb24"))
        case = qt.golden_case(SMALL)[0]
        want = qt.expected(raster, case[1], 3)
        assert ssim.tolist() == want[0] and sse.tolist() == want[1]
        assert C.string_at(slab, stride) == b"".join(p.tobytes() for p in raster)
    finally:
        gpu_ctx.sync()
        gpu_ctx.pinned_free(slab)
