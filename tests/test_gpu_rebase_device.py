"""The rebase with the new frame's records compacted and kept on the GPU (aa_rebase_device_batch / Context.rebase( records=False ); needs a
real MI355X): k_rebase_count and k_rebase_compact behind the two rebase kernels, the frame in a piece of HBM of its own.

Two references.  The reference's xc-enc -r on the fixtures of tests/golden/rebase, as tests/test_gpu_rebase.py uses them: the records
read back from the device-resident frame equal the parse of rebased.ivf, the decoded planes hash to rebase_golden.json, and frame by
frame rebase -> serialise -> decode writes rebased.ivf's bytes.  And aa_rebase_batch, the path from before this one, itself pinned to
xc-enc -r by that file: on twin decoders the 80-byte records and the coefficient blocks are equal as bytes -- on the fixtures (15
macroblocks at most: one workgroup of the scan) and on a 592 x 224 frame (37 x 14 = 518 macroblocks: two full runs of 256 and a tail of
6, a width that is no multiple of 4) made from a tools/vp8_synth.py stream with SPLITMV and intra macroblocks in its inter frames."""
import hashlib

import numpy as np
import pytest

import alfalfa_amd as aa
import rebase_model as rm
from alfalfa_amd import capi
from test_gpu_rebase import BATCH, compare_records, device_target, fixture_of, fresh_decoder

pytestmark = pytest.mark.gpu

_both, _big, _big_single = {}, {}, {}


def both(ctx, name):
    """Every frame of a case on twin decoders, the new call on one and aa_rebase_batch on the other -> per frame a dict; made once per
    context and case."""
    key = (ctx.h.value if hasattr(ctx.h, "value") else ctx.h, name)
    if key not in _both:
        case, pred, rebased, _ = fixture_of(name)
        new, old = fresh_decoder(ctx, case), fresh_decoder(ctx, case)
        out = []
        for k, (hdr, _, _) in enumerate(rebased):
            target = device_target(ctx, case["targets"][k])
            fi_new, count = new.rebase(hdr, pred[k + 1][1], target, records=False)
            fi_old, mb_ret, blocks_ret = old.rebase(hdr, pred[k + 1][1], target)
            got_new, got_old = new.read_records(fi_new), old.read_records(fi_old)
            ctx.decode_batch([new, old], [fi_new, fi_old])
            out.append(dict(count=count, new=got_new, old=got_old, returned=(mb_ret, blocks_ret), raster_new=new.raster_bytes(fi_new), raster_old=old.raster_bytes(fi_old),
                            header_new=new.frame_header(fi_new), header_old=old.frame_header(fi_old)))
        _both[key] = out
    return _both[key]


@pytest.mark.parametrize("name", rm.CASES)
def test_device_records_equal_the_reference(gpu_ctx, name):
    case, _, rebased, want_dense = fixture_of(name)
    for k, r in enumerate(both(gpu_ctx, name)):
        hdr, mb, blocks = r["new"]
        msg = compare_records("%s frame %d" % (name, k), mb, blocks, rebased[k][1], want_dense[k])
        assert msg is None, msg
        assert hashlib.sha256(r["raster_new"]).hexdigest() == case["sha256"][k], "%s frame %d: the decoded planes do not hash to the golden" % (name, k)
        assert r["count"] == len(blocks) == hdr["num_coeff_blocks"]
        for field in ("num_coeff_blocks", "num_intra_mbs", "has_intra_mb", "key_frame", "num_macroblocks"):
            assert r["header_new"][field] == r["header_old"][field], (name, k, field)


@pytest.mark.parametrize("name", rm.CASES)
def test_twin_decoders_old_call_and_new_call_hold_the_same_bytes(gpu_ctx, name):
    for k, r in enumerate(both(gpu_ctx, name)):
        (_, mb_new, blocks_new), (_, mb_old, blocks_old) = r["new"], r["old"]
        assert mb_new.tobytes() == mb_old.tobytes() == np.ascontiguousarray(r["returned"][0]).tobytes(), "%s frame %d: the 80-byte records differ" % (name, k)
        assert blocks_new.tobytes() == blocks_old.tobytes() == r["returned"][1].tobytes(), "%s frame %d: the coefficient blocks differ" % (name, k)
        assert r["raster_new"] == r["raster_old"]


# ---- a frame of 518 macroblocks ----
BIG_W, BIG_H = 592, 224
# A header may carry any factors: with all six at 30000 no coefficient of an 8-bit residue survives the division (the largest, a Y2 DC,
# stays below 2^15), so a target that is the frame's own reconstruction -- whose residues at the stream's own quantiser are NOT zero: they
# are the frame's -- stores nothing.  (The issue's fallback: "a quantiser at which it does".)
NOTHING_LEFT = [30000] * 6


def big(ctx):
    """-> (the stream's first two frames, the third frame's header and records, the decoded third frame's planes); once per context"""
    key = ctx.h.value if hasattr(ctx.h, "value") else ctx.h
    if key not in _big:
        import vp8_synth
        frames = vp8_synth.perf_stream(BIG_W, BIG_H, 41, 3).frames
        p = aa.Parser(BIG_W, BIG_H)
        hdr, mb, _ = [p.parse(fr) for fr in frames][2]
        assert mb.shape == (14, 37) and (mb["y_mode"] == rm.SPLITMV).any() and (mb["ref_frame"] == 0).any() and (mb["y_mode"] == rm.B_PRED).any()
        assert not hdr["key_frame"] and not hdr["segmentation_enabled"]
        d = aa.Decoder(ctx, BIG_W, BIG_H)
        for fr in frames:
            _, fi = d.get_frame_output(fr)
        _big[key] = (frames[:2], hdr, mb, [pl.copy() for pl in d.raster(fi)])
    return _big[key]


def big_decoder(ctx):
    d = aa.Decoder(ctx, BIG_W, BIG_H)
    for fr in big(ctx)[0]:
        d.get_frame_output(fr)
    return d


def big_job(ctx, which):
    """-> (header, prediction records, target planes) of target a (noise, low index), b (noise, high index) or c (own reconstruction)"""
    _, hdr, mb, planes = big(ctx)
    if which == "c":
        return dict(hdr, quant=[NOTHING_LEFT] * 4), mb, planes
    rng = np.random.default_rng(5)
    noisy = [np.clip(pl.astype(np.int32) + rng.integers(-12, 13, pl.shape), 0, 255).astype(np.uint8) for pl in planes]
    qi = 4 if which == "a" else 127
    return dict(hdr, q_index=qi, quant=[capi.quant_factors(qi)] * 4), mb, noisy


def big_single(ctx, which):
    """Target `which` through both calls on twin decoders -> (records, blocks, raster) of the new call; compared with the old one's here."""
    key = (ctx.h.value if hasattr(ctx.h, "value") else ctx.h, which)
    if key not in _big_single:
        hdr, mb, planes = big_job(ctx, which)
        target = device_target(ctx, planes)
        new, old = big_decoder(ctx), big_decoder(ctx)
        fi_old, mb_old, blocks_old = old.rebase(hdr, mb, target)
        if which == "c":
            assert len(blocks_old) == 0, "the old path stores %d blocks for the frame's own reconstruction: the target proves nothing about empty frames" % len(blocks_old)
        fi_new, count = new.rebase(hdr, mb, target, records=False)
        print("592x224 target %s: %d blocks of %d slots" % (which, count, 25 * mb.size))
        h_new, mb_new, blocks_new = new.read_records(fi_new)
        assert count == len(blocks_old) == h_new["num_coeff_blocks"]
        assert mb_new.tobytes() == np.ascontiguousarray(mb_old).tobytes() == old.read_records(fi_old)[1].tobytes(), "target %s: the 80-byte records differ" % which
        assert blocks_new.tobytes() == blocks_old.tobytes(), "target %s: the coefficient blocks differ" % which
        ctx.decode_batch([new, old], [fi_new, fi_old])
        raster = new.raster_bytes(fi_new)
        assert raster == old.raster_bytes(fi_old), "target %s: the decoded planes differ" % which
        _big_single[key] = (mb_new, blocks_new, raster)
    return _big_single[key]


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_518_macroblocks_two_runs_and_a_tail(gpu_ctx, which):
    mb, blocks, _ = big_single(gpu_ctx, which)
    if which == "a":
        assert len(blocks) > 0.75 * 24 * mb.size, "the dense target stores only %d blocks" % len(blocks)
        assert (mb["nz_mask"].reshape(-1)[256:] != 0).any() and (mb["nz_mask"].reshape(-1)[512:] != 0).any()          # (the second run and the tail hold blocks)
    if which == "b":
        assert 0 < len(blocks) < len(big_single(gpu_ctx, "a")[1])
    if which == "c":
        assert len(blocks) == 0 and (mb["flags"] & 8).all()


# ---- batches and slices ----
def lock_step_device(ctx, names):
    fx = [fixture_of(n) for n in names]
    decs = [fresh_decoder(ctx, f[0]) for f in fx]
    got = [[] for _ in names]
    for k in range(max(len(f[2]) for f in fx)):
        live = [i for i, f in enumerate(fx) if k < len(f[2])]
        targets = [device_target(ctx, fx[i][0]["targets"][k]) for i in live]
        results = ctx.rebase([decs[i] for i in live], [fx[i][2][k][0] for i in live], [fx[i][1][k + 1][1] for i in live], targets, records=False)
        records = [decs[i].read_records(fi) for i, (fi, _) in zip(live, results)]
        ctx.decode_batch([decs[i] for i in live], [fi for fi, _ in results])
        for i, (fi, count), (_, mb, blocks) in zip(live, results, records):
            assert count == len(blocks)
            got[i].append((mb.tobytes(), blocks.tobytes(), decs[i].raster_bytes(fi)))
    return got


def single(ctx, name):
    return [(r["new"][1].tobytes(), r["new"][2].tobytes(), r["raster_new"]) for r in both(ctx, name)]


def test_batches_and_slices_equal_the_single_runs(gpu_ctx, monkeypatch):
    for i, got in enumerate(lock_step_device(gpu_ctx, BATCH)):
        assert got == single(gpu_ctx, BATCH[i]), "batch of five: %s differs from its single-decoder run" % BATCH[i]
    monkeypatch.setenv("ALFALFA_AMD_REBASE_SLICE_BYTES", "40000")             # (12 000 bytes of dense scratch a job: slices of three jobs and a last one of one)
    for i, got in enumerate(lock_step_device(gpu_ctx, BATCH + BATCH)):
        assert got == single(gpu_ctx, (BATCH + BATCH)[i]), "batch of ten in slices: copy %d of %s differs from its single-decoder run" % (i // 5, (BATCH + BATCH)[i])


def test_jobs_of_different_sizes_in_one_launch(gpu_ctx):
    case, pred, rebased, _ = fixture_of("dir_split_80x48")
    small, large = fresh_decoder(gpu_ctx, case), big_decoder(gpu_ctx)
    hdr, mb, planes = big_job(gpu_ctx, "a")
    results = gpu_ctx.rebase([small, large], [rebased[0][0], hdr], [pred[1][1], mb], [device_target(gpu_ctx, case["targets"][0]), device_target(gpu_ctx, planes)], records=False)
    records = [d.read_records(fi) for d, (fi, _) in zip((small, large), results)]
    gpu_ctx.decode_batch([small, large], [fi for fi, _ in results])
    want_small, want_large = single(gpu_ctx, "dir_split_80x48")[0], big_single(gpu_ctx, "a")
    assert (records[0][1].tobytes(), records[0][2].tobytes(), small.raster_bytes(results[0][0])) == want_small
    assert records[1][1].tobytes() == want_large[0].tobytes() and records[1][2].tobytes() == want_large[1].tobytes() and large.raster_bytes(results[1][0]) == want_large[2]


# ---- the chain: rebase -> serialise -> decode, nothing but bytes coming down ----
@pytest.mark.parametrize("name", ["dir_split_80x48", "enc_best_72x40"])
def test_chain_writes_the_reference_s_bytes(gpu_ctx, name):
    from test_gpu_serialize import chunk_plan
    case, plan = chunk_plan("rebase", name)
    d = fresh_decoder(gpu_ctx, case)
    for k, step in enumerate(plan):
        fi, _ = d.rebase(step[0], step[3], device_target(gpu_ctx, case["targets"][k]), records=False)
        data = d.serialize_frame(fi, step[0], step[1], advance_state=True, sub_modes=step[2], optimise=True)
        want = case["rebased"][k]
        assert data == want, "%s frame %d: %d bytes, the reference wrote %d; first difference at byte %d" % (
            name, k, len(data), len(want), next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), min(len(data), len(want))))
        d.decode_frame(fi)
        assert hashlib.sha256(d.raster_bytes(fi)).hexdigest() == case["sha256"][k]


# ---- a stream that mixes kinds ----
def test_a_stream_of_parsed_device_rebased_host_rebased_and_appended_frames(gpu_ctx):
    case, pred, rebased, _ = fixture_of("dir_split_80x48")
    assert pred[0][0]["key_frame"]

    def chain(first_rebase_on_device):
        d = aa.Decoder(gpu_ctx, case["w"], case["h"])
        fis = [d.parse_frame(case["pred"][0])[0]]                                                         # a parsed frame (the key frame: every reference is a frame of this stream)
        d.decode_frame(fis[0])
        for k, on_device in ((0, first_rebase_on_device), (1, False)):                                 # a device-rebased frame, a host-rebased frame
            fis.append(d.rebase(rebased[k][0], pred[k + 1][1], device_target(gpu_ctx, case["targets"][k]), records=on_device)[0])
            d.decode_frame(fis[-1])
        fis.append(d.append_records(dict(rebased[2][0]), rebased[2][1], rebased[2][2]))                  # an append_records frame
        d.decode_frame(fis[-1])
        return d, fis

    d, fis = chain(True)
    twin, twin_fis = chain(False)
    rasters = [d.raster_bytes(fi) for fi in fis]
    assert fis == [0, 1, 2, 3] and rasters == [twin.raster_bytes(fi) for fi in twin_fis], "the stream with a device-rebased frame decodes differently from its host-rebased twin"
    assert d.read_records(1)[1].tobytes() == twin.read_records(1)[1].tobytes()
    d.rewind_to(1)
    for fi in fis[1:]:
        d.decode_frame(fi)
    assert [d.raster_bytes(fi) for fi in fis] == rasters, "after rewind_to the second frame the stream decodes differently"
    d.release_staging()
    assert d.read_records(1)[1].tobytes() == twin.read_records(1)[1].tobytes()
    d.release_frame(1)
    with pytest.raises(aa.AlfalfaError) as e:
        d.read_records(1)
    assert "released" in e.value.message
    with pytest.raises(aa.AlfalfaError):
        d.serialize_frame(1, rebased[0][0], d.header_ext())
    fi, _ = d.rebase(rebased[3][0], pred[4][1], device_target(gpu_ctx, case["targets"][3]), records=False)
    assert fi == 4 and len(d.read_records(fi)[1])
    d.decode_frame(fi)
    d.release_before(fi + 1)
    for released in (2, 3, fi):
        with pytest.raises(aa.AlfalfaError) as e:
            d.read_records(released)
        assert "released" in e.value.message
    # ... and the stream goes on
    fi, _ = d.rebase(rebased[4][0], pred[5][1], device_target(gpu_ctx, case["targets"][4]), records=False)
    d.decode_frame(fi)
    assert fi == 5 and len(d.raster_bytes(fi))


# ---- memory ----
def test_200_rounds_hold_no_memory(gpu_ctx):
    """rebase( device ) -> decode -> release_before, 200 times on one decoder: the device's free bytes after round 50 and after round 200
    differ by no more than one slab of the pool, 256 MiB -- the pool's granularity, not a measurement."""
    case, pred, rebased, _ = fixture_of("dir_split_80x48")
    d = fresh_decoder(gpu_ctx, case)
    targets = [device_target(gpu_ctx, t) for t in case["targets"]]
    free = {}
    for r in range(1, 201):
        k = r % len(rebased)                                       # (frames of different block counts: pieces of different sizes)
        fi, _ = d.rebase(rebased[k][0], pred[k + 1][1], targets[k], records=False)
        d.decode_frame(fi)
        d.release_before(fi + 1)
        if r in (50, 200):
            gpu_ctx.sync()
            free[r] = gpu_ctx.memory()[0]
    print("free bytes after round 50: %d, after round 200: %d" % (free[50], free[200]))
    assert abs(free[50] - free[200]) <= 256 << 20


# ---- refusals ----
def test_refusals_leave_every_stream_as_it_was(gpu_ctx):
    import ctypes as C
    case, pred, rebased, _ = fixture_of("dir_split_16x16")
    hdr, mb = dict(rebased[0][0]), pred[1][1]
    target = device_target(gpu_ctx, case["targets"][0])
    good, other = fresh_decoder(gpu_ctx, case), fresh_decoder(gpu_ctx, case)

    def refused(kind, text, decs, hdrs, mbs, targets):
        before = [d.frame_count() for d in decs]
        with pytest.raises(aa.AlfalfaError) as e:
            gpu_ctx.rebase(decs, hdrs, mbs, targets, records=False)
        assert e.value.kind == kind and e.value.message.startswith("aa_rebase_device_batch: job 1:") and text in e.value.message, e.value
        assert [d.frame_count() for d in decs] == before, "a refused call appended a frame"

    # (the good job comes first in every call: it must not be appended either)
    refused("BadArgument", "key frame", [good, other], [hdr, dict(hdr, key_frame=1)], [mb, mb], [target, target])
    refused("Unsupported", "segmentation", [good, other], [hdr, dict(hdr, segmentation_enabled=1)], [mb, mb], [target, target])
    refused("BadArgument", "dimensions", [good, other], [hdr, dict(hdr, mb_width=hdr["mb_width"] + 1)], [mb, np.concatenate([mb, mb], 1)], [target, target])
    refused("BadArgument", "also job 0", [good, good], [hdr, hdr], [mb, mb], [target, target])
    pending = fresh_decoder(gpu_ctx, case)
    pending.append_records(dict(rebased[0][0]), rebased[0][1], rebased[0][2])
    refused("LogicError", "not decoded", [good, pending], [hdr, hdr], [mb, mb], [target, target])
    pending_device = fresh_decoder(gpu_ctx, case)                  # ... and so does a device-rebased frame that was not decoded
    pending_device.rebase(hdr, mb, target, records=False)
    refused("LogicError", "not decoded", [good, pending_device], [hdr, hdr], [mb, mb], [target, target])
    foreign_ctx = aa.Context(gpu_ctx.device)
    foreign = fresh_decoder(foreign_ctx, case)
    refused("BadArgument", "another context", [good, foreign], [hdr, hdr], [mb, mb], [target, target])
    del foreign, foreign_ctx

    # the C call itself: null pointers
    L = capi.lib()
    h = capi.FrameHeader()
    for n, _ in capi.FrameHeader._fields_:
        if n != "quant":
            setattr(h, n, hdr[n])
    for s in range(4):
        for k in range(6):
            h.quant[s][k] = hdr["quant"][s][k]
    rec = np.ascontiguousarray(mb).reshape(-1)

    def job(dec, **kw):
        j = capi.RebaseDeviceJob()
        j.stream, j.hdr, j.mbs = dec.h, C.pointer(h), rec.ctypes.data_as(C.c_void_p)
        j.target.y, j.target.u, j.target.v = (t.data_ptr() for t in target)
        j.target.y_stride, j.target.uv_stride = case["pw"], case["pw"] // 2
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    for broken in (job(other, mbs=None), job(other, hdr=None), job(other, stream=None)):
        jobs = (capi.RebaseDeviceJob * 2)(job(good), broken)
        assert L.aa_rebase_device_batch(gpu_ctx.h, jobs, 2) == -7 and b"aa_rebase_device_batch: job 1: null pointer" in L.aa_last_error(), L.aa_last_error()
    no_plane = job(other)
    no_plane.target.u = None
    jobs = (capi.RebaseDeviceJob * 2)(job(good), no_plane)
    assert L.aa_rebase_device_batch(gpu_ctx.h, jobs, 2) == -7 and b"null pointer" in L.aa_last_error()
    assert L.aa_rebase_device_batch(gpu_ctx.h, None, 1) == -7
    assert good.frame_count() == 0 and other.frame_count() == 0
    # ... and the same two decoders are still good for a call that is
    jobs = (capi.RebaseDeviceJob * 2)(job(good), job(other))
    assert L.aa_rebase_device_batch(gpu_ctx.h, jobs, 2) == 0, L.aa_last_error()
    assert (jobs[0].frame_index, jobs[1].frame_index) == (0, 0) and jobs[0].num_coeff_blocks == jobs[1].num_coeff_blocks > 1
    assert good.read_records(0)[1].tobytes() == other.read_records(0)[1].tobytes()
