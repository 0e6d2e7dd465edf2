"""Batched hashes (Context.decoder_hashes / raster_hashes / minihashes -> aa_hash_decoders_async / aa_hash_rasters_async /
aa_ctx_hash_wait, k_hash_chains): one GPU lane per chain, no download.  Every expected value is the reference's own
(tests/golden/hash_golden.json) or the per-stream host route's (Decoder.raster_hash / decoder_hash of a decoder no batch call touched)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import alfalfa_amd as aa
from conftest import GOLDEN_DIR, ROOT, golden_frames

pytestmark = pytest.mark.gpu

HASHES = json.load(open(os.path.join(GOLDEN_DIR, "hash_golden.json")))
NAMES = sorted(HASHES)
_frames = {}


def frames_of(name):
    if name not in _frames:
        _frames[name] = golden_frames(name)
    return _frames[name]


def golden_at(name, i):
    g = HASHES[name]
    return [g["state"][i], g["last"][i], g["golden"][i], g["alternative"][i]], g["hash"][i], g["minihash"][i]


def reference_slots(d):
    slots = (C.c_int * 3)()
    aa.capi.check(d.L.aa_stream_reference_slots(d.h, slots))
    return list(slots)


def step(ctx, decoders, frames, device=()):
    """One frame for each decoder: decoders[i], i in `device`, through the GPU parser, the others through the host's; a decode_batch each."""
    dev = [i for i in range(len(decoders)) if i in device]
    host = [i for i in range(len(decoders)) if i not in device]
    if dev:
        ctx.decode_batch([decoders[i] for i in dev], ctx.submit_frames([(decoders[i], frames[i]) for i in dev], route="device"))
    if host:
        ctx.decode_batch([decoders[i] for i in host], [decoders[i].parse_frame(frames[i])[0] for i in host])


def lockstep(ctx, names, check):
    """All streams of `names` in lock step, odd ones through the GPU parser; check(alive, frame number) after every frame index."""
    streams = [frames_of(n) for n in names]
    decoders = [aa.Decoder(ctx, w, h) for w, h, _ in streams]
    for t in range(max(len(f) for _, _, f in streams)):
        alive = [i for i, (_, _, f) in enumerate(streams) if t < len(f)]
        step(ctx, [decoders[i] for i in alive], [streams[i][2][t] for i in alive], device={k for k, i in enumerate(alive) if i % 2})
        check([(names[i], decoders[i]) for i in alive], t)
    return decoders


def test_all_golden_streams_in_one_call_per_frame_index(gpu_ctx):
    """12 streams from 33x17 to 352x288, half host-parsed and half device-parsed: before the first frame every decoder's references
    are the context's blank raster of its size (one chain per size); after every frame index one decoder_hashes / minihashes over
    the decoders still running equals the reference's values: mixed sizes, segment maps with rows of 3 to 13 bytes at any
    alignment, 1, 2 and 3 distinct references."""
    ctx = gpu_ctx
    fresh = [aa.Decoder(ctx, w, h) for w, h, _ in map(frames_of, NAMES)]
    ctx.hash_stats(reset=True)
    got = ctx.decoder_hashes(fresh)
    st = ctx.hash_stats()
    sizes = {(d.padded_width, d.padded_height) for d in fresh}
    assert st["chains"] == len(sizes) < len(fresh) and st["cache_hits"] == 0, st
    host = [aa.Decoder(ctx, d.width, d.height).decoder_hash() for d in fresh]           # the host route, decoders no batch call saw
    assert got == host

    seen = []

    def check(alive, t):
        ds = [d for _, d in alive]
        got, mini = ctx.decoder_hashes(ds), ctx.minihashes(ds)
        for (name, _), (parts, whole), m in zip(alive, got, mini):
            want = golden_at(name, t)
            assert (parts, whole, m) == want, (name, t)
        seen.append(len(alive))

    lockstep(ctx, NAMES, check)
    assert seen[0] == 12 and len(seen) == 12 and seen[-1] == 1


def test_lanes_of_unequal_chains_share_a_wave(monkeypatch):
    """ALFALFA_AMD_HASH_SIMDS=4: the host plans as for a chip of four SIMDs, so the 12 streams' chains -- rasters of 1.5 KB to 150 KB
    and segment maps of 600 to 25 000 steps -- ride 4 to 8 lanes to a wave, longest first; the values are the reference's."""
    monkeypatch.setenv("ALFALFA_AMD_HASH_SIMDS", "4")
    ctx = aa.Context(0)
    calls = []

    def check(alive, t):
        before = ctx.hash_stats()["chains"]
        got = ctx.decoder_hashes([d for _, d in alive])
        calls.append(ctx.hash_stats()["chains"] - before)
        for (name, _), (parts, whole) in zip(alive, got):
            assert (parts, whole) == golden_at(name, t)[:2], (name, t)

    lockstep(ctx, NAMES, check)
    assert max(calls) >= 16, calls                                     # (at least four lanes to a wave in the fullest call)


def test_raster_hashes_equal_the_host_route(gpu_ctx):
    """raster_hashes of every decoded frame of four streams, in one call == Decoder.raster_hash of a second decoder of the stream that
    never saw a batch call (download + host chain); and == the reference's `last` where the frame became the last reference."""
    ctx = gpu_ctx
    names = ["synth_33x17_s7", "synth_175x143_s3", "qcif_q30_lf24", "w200_q40_lf63s7"]
    ds, fis, want, pinned = [], [], [], 0
    for name in names:
        w, h, frames = frames_of(name)
        a, b = aa.Decoder(ctx, w, h), aa.Decoder(ctx, w, h)
        for i, fr in enumerate(frames):
            fa, fb = a.parse_frame(fr)[0], b.parse_frame(fr)[0]
            ctx.decode_batch([a, b], [fa, fb])
            ds.append(a); fis.append(fa); want.append(b.raster_hash(fb))
            if a.get_references()["last"] == fa:
                assert want[-1] == HASHES[name]["last"][i], (name, i)
                pinned += 1
    ctx.hash_stats(reset=True)
    assert ctx.raster_hashes(ds, fis) == want
    assert ctx.hash_stats()["chains"] == len(ds) and pinned >= len(names)
    assert [d.raster_hash(fi) for d, fi in zip(ds, fis)] == want       # (now from the cache the wait filled)


def advance(ctx, name, targets):
    """len(targets) decoders of `name`, decoder k decoded up to and including frame targets[k], in lock step -> decoders"""
    w, h, frames = frames_of(name)
    ds = [aa.Decoder(ctx, w, h) for _ in targets]
    for t in range(max(targets) + 1):
        alive = [d for d, k in zip(ds, targets) if t <= k]
        step(ctx, alive, [frames[t]] * len(alive))
    return ds


def test_eighty_decoders_more_than_one_wave_and_the_cache(gpu_ctx):
    """80 decoders of s64_q5_rt at different frames in one call: every result is the reference's, chains launched = distinct device
    rasters (golden is often the raster last is), not 240.  A second identical call launches nothing; the per-stream calls then
    return the same values."""
    ctx = gpu_ctx
    name = "s64_q5_rt"
    n_frames = len(frames_of(name)[2])
    targets = [k % n_frames for k in range(80)]
    ds = advance(ctx, name, targets)
    distinct = sum(len(set(reference_slots(d))) for d in ds)
    assert 80 < distinct < 240
    ctx.hash_stats(reset=True)
    got = ctx.decoder_hashes(ds)
    st = ctx.hash_stats()
    assert st["chains"] == distinct and st["cache_fills"] == distinct and st["cache_hits"] == 0, st
    assert st["bytes"] == distinct * 64 * 64 * 3 // 2
    for k, (parts, whole) in zip(targets, got):
        assert (parts, whole) == golden_at(name, k)[:2], k
    assert ctx.minihashes(ds) == [golden_at(name, k)[2] for k in targets]
    # the cache: nothing is launched again, every distinct raster is answered from its Slot
    ctx.hash_stats(reset=True)
    assert ctx.decoder_hashes(ds) == got
    st = ctx.hash_stats()
    assert st["chains"] == 0 and st["cache_hits"] == distinct, st
    for d, g in zip(ds[:12], got[:12]):
        assert d.decoder_hash() == g and d.minihash() == g[1] & 0xFFFFFFFF
    assert ctx.hash_stats()["cache_hits"] >= distinct


def test_release_under_a_pending_call(gpu_ctx):
    """raster_hashes( wait=False ), then the frames are released and six more decoded on the same streams -- the pool would hand the
    rasters out again, were they not held by the call: the results are the values the host route gave before the call, and the new
    frames hash to the reference's values, not to the old ones."""
    ctx = gpu_ctx
    names = ["s64_q5_rt", "synth_64x64_s20"]
    ds, twins, held, want = [], [], [], []
    for name in names:
        w, h, frames = frames_of(name)
        a, b = aa.Decoder(ctx, w, h), aa.Decoder(ctx, w, h)          # b: the same stream, never part of a batch call
        for fr in frames[:2]:
            fa, fb = a.parse_frame(fr)[0], b.parse_frame(fr)[0]
            ctx.decode_batch([a, b], [fa, fb])
            held.append((a, fa)); want.append(b.raster_hash(fb))
        ds.append(a); twins.append(b)
    pending = ctx.raster_hashes([d for d, _ in held], [fi for _, fi in held], wait=False)
    for d, fi in held:
        d.release_frame(fi)
    last = {}
    for t in range(2, 8):
        for d, name in zip(ds, names):
            last[name] = d.parse_frame(frames_of(name)[2][t])[0]
        ctx.decode_batch(ds, [last[n] for n in names])
        ctx.decode_batch(twins, [b.parse_frame(frames_of(name)[2][t])[0] for b, name in zip(twins, names)])
    assert pending.result() == want
    assert pending.result() == want                                      # (a second look does not wait again)
    got = ctx.decoder_hashes(ds)
    for name, (parts, whole) in zip(names, got):
        assert (parts, whole) == golden_at(name, 7)[:2], name
    new = ctx.raster_hashes(ds, [last[n] for n in names])
    assert not set(new) & set(want)
    assert new == [b.raster_hash(last[name]) for b, name in zip(twins, names)]


def test_argument_and_state_errors(gpu_ctx):
    """Each refusal is of the per-stream call's kind, and a correct call works afterwards."""
    ctx = gpu_ctx
    name = "qcif_q30"
    w, h, frames = frames_of(name)
    d = aa.Decoder(ctx, w, h)
    f0 = d.parse_frame(frames[0])[0]

    def kind(fn):
        with pytest.raises(aa.AlfalfaError) as e:
            fn()
        return e.value.kind

    # parsed, not yet submitted
    assert kind(lambda: ctx.raster_hashes([d], [f0])) == kind(lambda: d.raster_hash(f0)) == "LogicError"
    assert kind(lambda: ctx.decoder_hashes([d])) == kind(d.decoder_hash) == "LogicError"
    assert kind(lambda: ctx.minihashes([d])) == kind(d.minihash) == "LogicError"
    ctx.decode_batch([d], [f0])
    assert kind(lambda: ctx.raster_hashes([d], [5])) == kind(lambda: d.raster_hash(5)) == "BadArgument"
    f1 = d.parse_frame(frames[1])[0]
    ctx.decode_batch([d], [f1])
    d.release_frame(f0)
    assert kind(lambda: ctx.raster_hashes([d, d], [f1, f0])) == kind(lambda: d.raster_hash(f0)) == "LogicError"
    # n = 0, lengths, another context's decoder
    with pytest.raises(ValueError):
        ctx.raster_hashes([], [])
    with pytest.raises(ValueError):
        ctx.decoder_hashes([])
    with pytest.raises(ValueError):
        ctx.raster_hashes([d], [f1, f1])
    other = aa.Decoder(aa.Context(0), w, h)
    with pytest.raises(ValueError):
        ctx.decoder_hashes([d, other])
    arr = (C.c_void_p * 2)(d.h, other.h)
    out = (C.c_uint64 * 8)()
    L = ctx.L
    assert L.aa_hash_decoders_async(ctx.h, arr, 0, out, None, None) == -7
    assert L.aa_hash_decoders_async(ctx.h, arr, 2, out, None, None) == -7
    assert L.aa_hash_rasters_async(ctx.h, arr, 2, (C.c_int * 2)(f1, 0), out) == -7
    assert L.aa_hash_rasters_async(ctx.h, arr, 0, (C.c_int * 2)(f1, 0), out) == -7
    # ... and none of it left anything behind
    assert ctx.decoder_hashes([d]) == [golden_at(name, 1)[:2]]
    assert ctx.raster_hashes([d], [f1]) == [golden_at(name, 1)[0][1]]
    assert ctx.minihashes([d]) == [golden_at(name, 1)[2]]


def test_seventeen_outstanding_calls(gpu_ctx):
    """The ring of 16 buffers wraps: the 17th call commits the oldest, every call's result is right."""
    ctx = gpu_ctx
    name = "synth_96x80_s1"                      # segmentation on after every frame: a map chain per call
    n_frames = len(frames_of(name)[2])
    targets = [k % n_frames for k in range(20)]
    ds = advance(ctx, name, targets)
    ctx.hash_wait()
    ctx.hash_stats(reset=True)
    pending = [ctx.decoder_hashes([d], wait=False) for d in ds]
    assert ctx.hash_stats()["cache_fills"] > 0                            # (the first calls were committed to make room)
    for k, p in zip(targets, pending):
        assert p.result() == [golden_at(name, k)[:2]], k


CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import alfalfa_amd as aa
from conftest import golden_frames
w, h, frames = golden_frames("qcif_q30")
ctx = aa.Context(0)
ds = [aa.Decoder(ctx, w, h) for _ in range(3)]
for d in ds:
    d.get_frame_output(frames[0])
pending = [ctx.decoder_hashes([d], wait=False) for d in ds] + [ctx.raster_hashes(ds, [0, 0, 0], wait=False)]
del ds[0]                  # a stream destroyed with calls outstanding
del d
del pending, ds, ctx       # ... and the context
import gc
gc.collect()
print("DESTROYED")
'''


def test_destruction_with_calls_outstanding_completes():
    """A decoder and then the context destroyed with hash calls outstanding: both commit them first.  In a child process with a time
    limit: anything that could wait for good must not take the suite with it."""
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "DESTROYED"
