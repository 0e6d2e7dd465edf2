"""The re-encode with the new frame's records compacted and kept on the GPU (aa_reencode_device_batch / Context.reencode_as_inter(
records=False ); needs a real MI355X): k_reencode_count and k_reencode_compact behind k_reencode_inter, the frame in a piece of HBM of
its own.

Two references.  The reference's xc-enc -r on the fixtures of tests/golden/reencode, as tests/test_gpu_reencode.py uses them: the
records read back from the device-resident frame equal the parse of rebased.ivf (lf_level, segment_id and coeff_index too), the decoded
planes hash to reencode_golden.json, and a whole chunk -- frame 0 re-encoded, the others rebased, every frame kept on the device,
serialised and decoded -- writes rebased.ivf's bytes.  And aa_reencode_batch, the path from before this one, itself pinned to xc-enc -r
by that file: on twin decoders the 80-byte records and the coefficient blocks are equal as bytes -- on the fixtures (25 macroblocks at
most: one workgroup of the scan) and on a 592 x 224 frame (37 x 14 = 518 macroblocks: two full runs of 256 and a tail of 6, rows of 37
that straddle both run boundaries) whose target mixes stripes of the stream's own next picture with stripes of unrelated pictures, so
that every run holds intra and inter macroblocks."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import alfalfa_amd as aa
import reencode_model as rmm
from alfalfa_amd import capi
from test_gpu_rebase import device_target
from test_gpu_rebase_device import BIG_H, BIG_W, NOTHING_LEFT, big, big_decoder
from test_gpu_reencode import check_frame0, fresh_decoder, wanted

pytestmark = pytest.mark.gpu

_both, _big_both = {}, {}


def key_of(ctx):
    return ctx.h.value if hasattr(ctx.h, "value") else ctx.h


def both(ctx, name):
    """A case's frame 0 on twin decoders, the new call on one and aa_reencode_batch on the other -> dict; made once per context and case."""
    key = (key_of(ctx), name)
    if key not in _both:
        case = rmm.load_case(name)
        hdr = wanted(name)[0][0]
        target = device_target(ctx, case["targets"][0])
        new, old = fresh_decoder(ctx, case), fresh_decoder(ctx, case)
        fi_new, count = new.reencode_as_inter(hdr, target, quality=case["quality"], records=False)
        fi_old, mb_ret, blocks_ret = old.reencode_as_inter(hdr, target, quality=case["quality"])
        assert fi_new == fi_old == 0 and new.frame_count() == 1
        got_new, got_old = new.read_records(fi_new), old.read_records(fi_old)
        ctx.decode_batch([new, old], [fi_new, fi_old])
        _both[key] = dict(count=count, new=got_new, old=got_old, returned=(mb_ret, blocks_ret), raster_new=new.raster_bytes(fi_new), raster_old=old.raster_bytes(fi_old),
                          header_new=new.frame_header(fi_new), header_old=old.frame_header(fi_old))
    return _both[key]


# ---- 1. the reference ----
@pytest.mark.parametrize("name", rmm.CASES)
def test_device_records_equal_the_reference(gpu_ctx, name):
    r = both(gpu_ctx, name)
    hdr, mb, blocks = r["new"]
    check_frame0(name, mb, blocks)             # compare_records against the parse of rebased.ivf, then u, lf_level, segment_id, coeff_index
    assert hashlib.sha256(r["raster_new"]).hexdigest() == rmm.load_case(name)["sha256"][0], "%s frame 0: the decoded planes do not hash to the golden" % name
    assert r["count"] == len(blocks) == hdr["num_coeff_blocks"]
    for field in ("num_coeff_blocks", "num_intra_mbs", "has_intra_mb", "key_frame", "num_macroblocks"):
        assert r["header_new"][field] == r["header_old"][field], (name, field)
    assert r["header_new"]["num_intra_mbs"] == int((mb["ref_frame"] == 0).sum())


# ---- 2. twin decoders ----
@pytest.mark.parametrize("name", rmm.CASES)
def test_twin_decoders_old_call_and_new_call_hold_the_same_bytes(gpu_ctx, name):
    r = both(gpu_ctx, name)
    (_, mb_new, blocks_new), (_, mb_old, blocks_old) = r["new"], r["old"]
    assert mb_new.tobytes() == mb_old.tobytes() == np.ascontiguousarray(r["returned"][0]).tobytes(), "%s: the 80-byte records differ" % name
    assert blocks_new.tobytes() == blocks_old.tobytes() == r["returned"][1].tobytes(), "%s: the coefficient blocks differ" % name
    assert r["raster_new"] == r["raster_old"]


# ---- a frame of 518 macroblocks ----
STRIPE = 32        # luma columns: two macroblocks of the stream's own picture, two of a foreign one, ...


def foreign_pictures(w, h):
    """Two pictures nothing in the stream predicts: a smooth ramp (a 16 x 16 intra predictor does well there) and a texture of oblique
    edges on a ramp (the 4 x 4 predictors of B_PRED do better) -> [(y, u, v)] * 2, of the padded plane shapes."""
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    ramp = (((xx * 3 + yy * 5) // 4) % 224 + 16).astype(np.uint8), ((cx * 2 + cy) % 160 + 48).astype(np.uint8), ((cx + cy * 3) % 160 + 48).astype(np.uint8)
    edges = np.where(((xx + 2 * yy) // 5) % 2 == 0, 40 + (yy % 64), 200 - (xx % 64)).astype(np.uint8)
    texture = edges, ((cx * 5 + cy * 2) % 128 + 64).astype(np.uint8), ((cx * 3) % 128 + 64).astype(np.uint8)
    return [ramp, texture]


def big_target(planes):
    """The decoded third frame in vertical stripes of STRIPE luma columns, every other stripe replaced by a foreign picture (ramp and
    texture in turn) -> (y, u, v)."""
    h, w = planes[0].shape
    foreign = foreign_pictures(w, h)
    out = [p.copy() for p in planes]
    for s in range(1, (w + STRIPE - 1) // STRIPE, 2):
        src = foreign[(s // 2) % 2]
        for p in range(3):
            lo, hi = (s * STRIPE, (s + 1) * STRIPE) if p == 0 else (s * STRIPE // 2, (s + 1) * STRIPE // 2)
            out[p][:, lo:hi] = src[p][:, lo:hi]
    return tuple(out)


def census_of(mb, quality):
    """What the 592 x 224 target must make of the old path's records, or the message that names what is missing."""
    flat = mb.reshape(-1)
    missing = []
    for run, (lo, hi) in enumerate(((0, 256), (256, 512), (512, 518))):
        if not (flat["ref_frame"][lo:hi] == 0).any():
            missing.append("no intra macroblock in run %d" % run)
        if not (flat["ref_frame"][lo:hi] != 0).any():
            missing.append("no inter macroblock in run %d" % run)
    if quality == "best" and not (flat["y_mode"] == rmm.B_PRED).any():
        missing.append("no B_PRED macroblock under -q best")
    return missing


def reference_raster(ctx):
    """-> the planes of the LAST reference of big_decoder: the stream's second frame"""
    key = ("reference", key_of(ctx))
    if key not in _big_both:
        d = big_decoder(ctx)
        _big_both[key] = [p.copy() for p in d.raster(d.frame_count() - 1)]
    return _big_both[key]


def big_job(ctx, which):
    """-> (header, target planes, quality) of job "best" / "rt" (the striped target) or "nothing" (every factor 30000, target = reference)"""
    _, hdr, _, planes = big(ctx)
    if which == "nothing":
        return dict(hdr, quant=[NOTHING_LEFT] * 4), reference_raster(ctx), "best"
    return hdr, big_target(planes), which


def big_both(ctx, which):
    """Job `which` through both calls on twin decoders -> (records, blocks, raster) of the new call; compared with the old one's here."""
    key = (key_of(ctx), which)
    if key not in _big_both:
        hdr, planes, quality = big_job(ctx, which)
        target = device_target(ctx, planes)
        new, old = big_decoder(ctx), big_decoder(ctx)
        fi_old, mb_old, blocks_old = old.reencode_as_inter(hdr, target, quality=quality)
        if which == "nothing":
            assert len(blocks_old) == 0, "the old path stores %d blocks for the reference itself at factors of 30000: the job proves nothing about empty frames" % len(blocks_old)
        else:
            missing = census_of(mb_old, quality)
            assert not missing, "the 592 x 224 target does not exercise the compaction, on the old path's records: " + "; ".join(missing)
        fi_new, count = new.reencode_as_inter(hdr, target, quality=quality, records=False)
        print("592x224 job %s: %d blocks of %d slots, %d intra macroblocks, %d B_PRED" % (which, count, 25 * mb_old.size, int((mb_old["ref_frame"] == 0).sum()),
                                                                                          int((mb_old["y_mode"] == rmm.B_PRED).sum())))
        h_new, mb_new, blocks_new = new.read_records(fi_new)
        h_old = old.frame_header(fi_old)
        assert count == len(blocks_old) == h_new["num_coeff_blocks"]
        assert (h_new["num_intra_mbs"], h_new["has_intra_mb"]) == (h_old["num_intra_mbs"], h_old["has_intra_mb"]) == (int((mb_old["ref_frame"] == 0).sum()), int((mb_old["ref_frame"] == 0).any()))
        assert mb_new.tobytes() == np.ascontiguousarray(mb_old).tobytes() == old.read_records(fi_old)[1].tobytes(), "job %s: the 80-byte records differ" % which
        assert blocks_new.tobytes() == blocks_old.tobytes(), "job %s: the coefficient blocks differ" % which
        ctx.decode_batch([new, old], [fi_new, fi_old])
        raster = new.raster_bytes(fi_new)
        assert raster == old.raster_bytes(fi_old), "job %s: the decoded planes differ" % which
        _big_both[key] = (mb_new, blocks_new, raster)
    return _big_both[key]


@pytest.mark.parametrize("which", ["best", "rt", "nothing"])
def test_518_macroblocks_two_runs_and_a_tail(gpu_ctx, which):
    mb, blocks, _ = big_both(gpu_ctx, which)
    assert mb.shape == (BIG_H // 16, BIG_W // 16) == (14, 37)
    if which == "nothing":
        assert len(blocks) == 0 and (mb["flags"] & 8).all() and (mb["nz_mask"] == 0).all()
    else:
        assert (mb["nz_mask"].reshape(-1)[256:512] != 0).any() and (mb["nz_mask"].reshape(-1)[512:] != 0).any()          # (the second run and the tail hold blocks)


# ---- 3. batches, capped rounds and slices ----
def all_in_one_call(ctx):
    """Every fixture and, beside the 16 x 16 one, the 518-macroblock frame, in ONE call -> [(records, blocks, raster)] in that order"""
    cases = [rmm.load_case(n) for n in rmm.CASES]
    decs = [fresh_decoder(ctx, c) for c in cases] + [big_decoder(ctx)]
    hdr, planes, quality = big_job(ctx, "best")
    headers = [wanted(n)[0][0] for n in rmm.CASES] + [hdr]
    targets = [device_target(ctx, c["targets"][0]) for c in cases] + [device_target(ctx, planes)]
    results = ctx.reencode_as_inter(decs, headers, targets, quality=[c["quality"] for c in cases] + [quality], records=False)
    records = [d.read_records(fi) for d, (fi, _) in zip(decs, results)]
    ctx.decode_batch(decs, [fi for fi, _ in results])
    for (fi, count), (_, mb, blocks) in zip(results, records):
        assert count == len(blocks)
    return [(mb.tobytes(), blocks.tobytes(), d.raster_bytes(fi)) for d, (fi, _), (_, mb, blocks) in zip(decs, results, records)]


def singles(ctx):
    out = [(both(ctx, n)["new"][1].tobytes(), both(ctx, n)["new"][2].tobytes(), both(ctx, n)["raster_new"]) for n in rmm.CASES]
    mb, blocks, raster = big_both(ctx, "best")
    return out + [(mb.tobytes(), blocks.tobytes(), raster)]


def test_one_call_capped_rounds_and_slices_equal_the_single_runs(gpu_ctx, monkeypatch):
    assert "best_16x16" in rmm.CASES          # (a 16 x 16 job and the 518-macroblock job share the launch)
    want = singles(gpu_ctx)
    names = rmm.CASES + ["592x224"]
    try:
        for slots in (16, 1, 2):
            gpu_ctx.set_reencode_slots(slots)
            for n, got, w in zip(names, all_in_one_call(gpu_ctx), want):
                assert got == w, "%d macroblocks per round, all jobs in one call: %s differs from its single run" % (slots, n)
    finally:
        gpu_ctx.set_reencode_slots(16)
    # (20 000 bytes of dense scratch for a 80 x 80 job, 12 000 for a 72 x 40 one, 414 400 for the large one: slices of two, four, one and one jobs)
    monkeypatch.setenv("ALFALFA_AMD_REBASE_SLICE_BYTES", "50000")
    for n, got, w in zip(names, all_in_one_call(gpu_ctx), want):
        assert got == w, "all jobs in one call, in slices: %s differs from its single run" % n


# ---- 4. the chain: re-encode -> rebase -> serialise -> decode, nothing but bytes coming down ----
@pytest.mark.parametrize("name", ["best_80x80", "rt_72x40"])
def test_chain_writes_the_reference_s_bytes(gpu_ctx, name):
    from test_gpu_serialize import chunk_plan
    case, plan = chunk_plan("reencode", name)
    d = fresh_decoder(gpu_ctx, case)
    for k, step in enumerate(plan):
        target = device_target(gpu_ctx, case["targets"][k])
        if k == 0:
            fi, _ = d.reencode_as_inter(step[0], target, quality=case["quality"], records=False)
        else:
            fi, _ = d.rebase(step[0], step[3], target, records=False)
        data = d.serialize_frame(fi, step[0], step[1], advance_state=True, sub_modes=step[2], optimise=True)
        want = case["rebased"][k]
        assert data == want, "%s frame %d: %d bytes, the reference wrote %d; first difference at byte %d" % (
            name, k, len(data), len(want), next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), min(len(data), len(want))))
        d.decode_frame(fi)
        assert hashlib.sha256(d.raster_bytes(fi)).hexdigest() == case["sha256"][k]


# ---- 5. the diagonal schedule ----
def test_the_diagonal_schedule_decodes_the_same_raster(gpu_ctx):
    """One launch per anti-diagonal runs the intra kernels only on the diagonals FrameRec::intra_diagonals names."""
    name = "bpred_72x40"
    r = both(gpu_ctx, name)
    assert r["header_new"]["num_intra_mbs"] > 0
    case = rmm.load_case(name)
    _, _, big_raster = big_both(gpu_ctx, "best")
    hdr, planes, quality = big_job(gpu_ctx, "best")
    small, large = fresh_decoder(gpu_ctx, case), big_decoder(gpu_ctx)
    results = gpu_ctx.reencode_as_inter([small, large], [wanted(name)[0][0], hdr], [device_target(gpu_ctx, case["targets"][0]), device_target(gpu_ctx, planes)],
                                        quality=[case["quality"], quality], records=False)
    try:
        gpu_ctx.set_schedule("diagonal")
        gpu_ctx.decode_batch([small, large], [fi for fi, _ in results])
        got = small.raster_bytes(results[0][0]), large.raster_bytes(results[1][0])
    finally:
        gpu_ctx.set_schedule("rows")
    assert got[0] == r["raster_new"], "%s: the diagonal schedule decodes the device-re-encoded frame differently" % name
    assert got[1] == big_raster, "592 x 224: the diagonal schedule decodes the device-re-encoded frame differently"


# ---- 6. lifetime ----
def test_rewind_release_and_the_stream_goes_on(gpu_ctx):
    """The re-encoded frame behind two parsed ones (a stream rewinds to a frame whose references are frames of its own), and a second
    re-encode predicted from the first."""
    hdr, planes, quality = big_job(gpu_ctx, "best")
    mb_want, _, raster_want = big_both(gpu_ctx, "best")
    target = device_target(gpu_ctx, planes)
    d = big_decoder(gpu_ctx)
    first = d.frame_count()
    fis = []
    for q in (quality, "rt"):
        fis.append(d.reencode_as_inter(hdr, target, quality=q, records=False)[0])
        d.decode_frame(fis[-1])
    assert fis == [first, first + 1]
    rasters = [d.raster_bytes(fi) for fi in fis]
    assert rasters[0] == raster_want
    d.rewind_to(fis[0])
    for fi in fis:
        d.decode_frame(fi)
    assert [d.raster_bytes(fi) for fi in fis] == rasters, "after rewind_to the re-encoded frame the stream decodes differently"
    d.release_staging()
    assert d.read_records(fis[0])[1].tobytes() == mb_want.tobytes()
    d.release_frame(fis[0])
    with pytest.raises(aa.AlfalfaError) as e:
        d.read_records(fis[0])
    assert "released" in e.value.message
    with pytest.raises(aa.AlfalfaError):
        d.serialize_frame(fis[0], hdr, d.header_ext())
    d.release_before(fis[1] + 1)
    with pytest.raises(aa.AlfalfaError) as e:
        d.read_records(fis[1])
    assert "released" in e.value.message
    # ... and the stream goes on
    fi, count = d.reencode_as_inter(hdr, target, quality=quality, records=False)
    d.decode_frame(fi)
    assert fi == first + 2 and count == len(d.read_records(fi)[2]) and len(d.raster_bytes(fi))


def test_200_rounds_hold_no_memory(gpu_ctx):
    """reencode( device ) -> decode -> release_before, 200 times on one decoder: the device's free bytes after round 50 and after round
    200 differ by no more than one slab of the pool, 256 MiB -- the pool's granularity, not a measurement."""
    names = ["best_80x80", "rt_80x80", "rt_low_80x80"]                 # (one size, different block counts: pieces of different sizes)
    cases = [rmm.load_case(n) for n in names]
    assert len({(c["w"], c["h"]) for c in cases}) == 1
    d = fresh_decoder(gpu_ctx, cases[0])
    targets = [device_target(gpu_ctx, c["targets"][0]) for c in cases]
    free = {}
    for r in range(1, 201):
        k = r % len(names)
        fi, _ = d.reencode_as_inter(wanted(names[k])[0][0], targets[k], quality=cases[k]["quality"], records=False)
        d.decode_frame(fi)
        d.release_before(fi + 1)
        if r in (50, 200):
            gpu_ctx.sync()
            free[r] = gpu_ctx.memory()[0]
    print("free bytes after round 50: %d, after round 200: %d" % (free[50], free[200]))
    assert abs(free[50] - free[200]) <= 256 << 20


# ---- 7. refusals ----
def test_refusals_leave_every_stream_as_it_was(gpu_ctx):
    name = "best_16x16"
    case = rmm.load_case(name)
    hdr = dict(wanted(name)[0][0])
    target = device_target(gpu_ctx, case["targets"][0])
    good, other = fresh_decoder(gpu_ctx, case), fresh_decoder(gpu_ctx, case)

    def refused(kind, text, decs, hdrs, targets):
        before = [d.frame_count() for d in decs]
        with pytest.raises(aa.AlfalfaError) as e:
            gpu_ctx.reencode_as_inter(decs, hdrs, targets, records=False)
        assert e.value.kind == kind and e.value.message.startswith("aa_reencode_device_batch: job 1:") and text in e.value.message, e.value
        assert [d.frame_count() for d in decs] == before, "a refused call appended a frame"

    # (the good job comes first in every call: it must not be appended either)
    refused("BadArgument", "key frame", [good, other], [hdr, dict(hdr, key_frame=1)], [target, target])
    refused("Unsupported", "segmentation", [good, other], [hdr, dict(hdr, segmentation_enabled=1)], [target, target])
    wide = rmm.load_case("best_72x40")
    refused("BadArgument", "dimensions", [good, fresh_decoder(gpu_ctx, wide)], [hdr, hdr], [target, device_target(gpu_ctx, wide["targets"][0])])
    refused("BadArgument", "also job 0", [good, good], [hdr, hdr], [target, target])
    pending = fresh_decoder(gpu_ctx, case)
    w = rmm.parsed(name, "rebased")[0]
    pending.append_records(dict(w[0]), w[1], w[2])
    refused("LogicError", "not decoded", [good, pending], [hdr, hdr], [target, target])
    pending_device = fresh_decoder(gpu_ctx, case)                  # ... and so does a device-made frame that was not decoded
    pending_device.reencode_as_inter(hdr, target, records=False)
    refused("LogicError", "not decoded", [good, pending_device], [hdr, hdr], [target, target])
    foreign_ctx = aa.Context(gpu_ctx.device)
    foreign = fresh_decoder(foreign_ctx, case)
    refused("BadArgument", "another context", [good, foreign], [hdr, hdr], [target, target])
    del foreign, foreign_ctx
    with pytest.raises(ValueError):
        gpu_ctx.reencode_as_inter([good], [hdr], [target], records=False, append=False)
    with pytest.raises(ValueError):
        good.reencode_as_inter(hdr, target, records=False, append=False)
    assert good.frame_count() == 0

    # the C call itself: null pointers and a quality that is none
    L = capi.lib()
    h = gpu_ctx._header_struct(hdr)

    def job(dec, **kw):
        j = capi.ReencodeDeviceJob()
        j.stream, j.hdr, j.quality = dec.h, C.pointer(h), 0
        j.target.y, j.target.u, j.target.v = (t.data_ptr() for t in target)
        j.target.y_stride, j.target.uv_stride = case["pw"], case["pw"] // 2
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    for broken in (job(other, hdr=None), job(other, stream=None)):
        jobs = (capi.ReencodeDeviceJob * 2)(job(good), broken)
        assert L.aa_reencode_device_batch(gpu_ctx.h, jobs, 2) == -7 and b"aa_reencode_device_batch: job 1: null pointer" in L.aa_last_error(), L.aa_last_error()
    no_plane = job(other)
    no_plane.target.u = None
    jobs = (capi.ReencodeDeviceJob * 2)(job(good), no_plane)
    assert L.aa_reencode_device_batch(gpu_ctx.h, jobs, 2) == -7 and b"null pointer" in L.aa_last_error()
    jobs = (capi.ReencodeDeviceJob * 2)(job(good), job(other, quality=2))
    assert L.aa_reencode_device_batch(gpu_ctx.h, jobs, 2) == -7 and b"aa_reencode_device_batch: job 1: quality" in L.aa_last_error(), L.aa_last_error()
    assert L.aa_reencode_device_batch(gpu_ctx.h, None, 1) == -7
    assert good.frame_count() == 0 and other.frame_count() == 0
    # ... and the same two decoders are still good for a call that is
    jobs = (capi.ReencodeDeviceJob * 2)(job(good), job(other))
    assert L.aa_reencode_device_batch(gpu_ctx.h, jobs, 2) == 0, L.aa_last_error()
    need = both(gpu_ctx, name)["count"]
    assert (jobs[0].frame_index, jobs[1].frame_index) == (0, 0) and jobs[0].num_coeff_blocks == jobs[1].num_coeff_blocks == need > 1
    assert jobs[0].num_intra_mbs == jobs[1].num_intra_mbs == both(gpu_ctx, name)["header_new"]["num_intra_mbs"]
    assert good.read_records(0)[1].tobytes() == other.read_records(0)[1].tobytes() == both(gpu_ctx, name)["new"][1].tobytes()
    timing = gpu_ctx.reencode_timing()
    assert timing["call_ms"] > 0 and timing["kernels_ms"] > 0 and timing["records_ms"] == 0
