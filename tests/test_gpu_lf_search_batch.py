"""The loop-filter level search of appended frames on the GPU, batched (aa_lf_search_decode_batch / Context.lf_search_decode; needs a real
MI355X): k_lf_candidates, k_lf_choose and k_lf_finish around the loop-filter and scoring kernels that exist.

The reference is xc-enc-ssim -r -- the reference's encoder with a real SSIM -- on the fixtures of tests/golden/lf_search: the level in the
header of frame 0 of rebased.ivf is the level its own search chose, lf_search_golden.json holds the oracle's score of every level, and the
chain re-encode -> search -> serialise must write rebased.ivf's bytes.  The seven fixtures of tests/golden/reencode were written under the
PSNR-like stub: measure "sse" finds their level 0."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import alfalfa_amd as aa
import lf_search_model as lm
import rebase_model as rm
import reencode_model as rmm
from alfalfa_amd import capi
from test_gpu_rebase import compare_records, device_target
from test_gpu_serialize import cleared, walk

pytestmark = pytest.mark.gpu

_memo = {}


def key_of(ctx):
    return ctx.h.value if hasattr(ctx.h, "value") else ctx.h


def fresh_decoder(ctx, case):
    d = aa.Decoder(ctx, case["w"], case["h"])
    d.deserialize(case["state"])
    return d


def append_wrong(d, name, parsed=lm.parsed):
    """Frame 0 of a case's rebased.ivf appended as records with a wrong level in the header and in every record -> frame index"""
    hdr, mb, blocks = parsed(name)[0]
    wrong = 63 - hdr["loop_filter_level"]
    mb2 = mb.copy()
    mb2["lf_level"] = wrong
    return d.append_records(dict(hdr, loop_filter_level=wrong), mb2, blocks)


def snapshot(d, fi):
    h, mb, blocks = d.read_records(fi)
    return (h["loop_filter_level"], h["filter_adjustments_enabled"], mb.tobytes(), blocks.tobytes(), d.raster_bytes(fi))


def searched(ctx, name):
    """A new case's frame 0 from the reference's records, searched alone over 0..63 -> dict; once per context and case."""
    key = (key_of(ctx), name)
    if key not in _memo:
        case = lm.load_case(name)
        d = fresh_decoder(ctx, case)
        fi = append_wrong(d, name)
        result = d.lf_search_decode(fi, device_target(ctx, case["targets"][0]))
        print(name, "->", result, ctx.lf_search_timing())
        _memo[key] = dict(result=result, snap=snapshot(d, fi), decoder=d, fi=fi)
    return _memo[key]


# ---- 1. records from the reference ----
@pytest.mark.parametrize("name", lm.CASES)
def test_records_from_the_reference(gpu_ctx, name):
    want_level, want_evaluated, _, _ = lm.REFERENCE[name]
    hdr, mb, blocks = lm.parsed(name)[0]
    assert hdr["loop_filter_level"] == want_level
    r = searched(gpu_ctx, name)
    best, score, evaluated = r["result"]
    assert (best, evaluated) == (want_level, want_evaluated)
    assert score == lm.ssim_table(name)[best], "%s: the score of level %d is %r, the oracle's %r" % (name, best, score, lm.ssim_table(name)[best])
    level, adjustments, mb_bytes, block_bytes, raster = r["snap"]
    assert hashlib.sha256(raster).hexdigest() == lm.load_case(name)["sha256"][0], "%s: the filtered planes do not hash to the golden" % name
    assert (level, adjustments) == (want_level, 1)
    assert mb_bytes == np.ascontiguousarray(mb).tobytes(), "%s: the records read back are not the parse of the reference's frame" % name
    assert block_bytes == blocks.tobytes()


# ---- 2. all five in one call: mixed geometry, jobs finishing in different rounds; K and the slicing change nothing ----
def all_in_one_call(ctx):
    cases = [lm.load_case(n) for n in lm.CASES]
    decs = [fresh_decoder(ctx, c) for c in cases]
    fis = [append_wrong(d, n) for d, n in zip(decs, lm.CASES)]
    results = ctx.lf_search_decode(decs, fis, [device_target(ctx, c["targets"][0]) for c in cases])
    return [(r, snapshot(d, fi)) for r, d, fi in zip(results, decs, fis)], ctx.lf_search_timing()["rounds"]


def test_one_call_whatever_the_round_and_the_slices(gpu_ctx):
    want = [(searched(gpu_ctx, n)["result"], searched(gpu_ctx, n)["snap"]) for n in lm.CASES]
    try:
        for levels, per_slice, rounds in ((4, 0, 6), (1, 0, 23), (3, 0, 8), (8, 0, 3), (4, 2, 6 + 5 + 5)):
            gpu_ctx.set_lf_search_round(levels, per_slice)
            got, ran = all_in_one_call(gpu_ctx)
            for n, g, w in zip(lm.CASES, got, want):
                assert g == w, "%d levels per round, %d jobs per slice: %s differs from its single run: %r, alone %r" % (levels, per_slice, n, g[0], w[0])
            assert ran == rounds, "%d levels per round, %d jobs per slice: %d rounds" % (levels, per_slice, ran)
    finally:
        gpu_ctx.set_lf_search_round(4, 0)


# ---- 3. ranges ----
@pytest.mark.parametrize("lo,hi", [(20, 22), (22, 63), (21, 21)])
def test_ranges(gpu_ctx, lo, hi):
    name = "ssim_rt_72x40"
    case = lm.load_case(name)
    d = fresh_decoder(gpu_ctx, case)
    fi = append_wrong(d, name)
    got = d.lf_search_decode(fi, device_target(gpu_ctx, case["targets"][0]), lo, hi)
    assert got == lm.rule(lm.ssim_table(name), lo, hi)
    if (lo, hi) == (20, 22):
        assert got[0] == 21 and got[2] == 3
    assert d.frame_header(fi)["loop_filter_level"] == got[0] and (d.read_records(fi)[1]["lf_level"] == got[0]).all()


# ---- 4. device-resident frames ----
@pytest.mark.parametrize("name", lm.CASES)
def test_device_resident_frames(gpu_ctx, name):
    case = lm.load_case(name)
    want_hdr, want_mb, want_blocks = lm.parsed(name)[0]
    hdr = dict(want_hdr, loop_filter_level=63 if want_hdr["loop_filter_level"] != 63 else 0)
    target = device_target(gpu_ctx, case["targets"][0])
    new, twin = fresh_decoder(gpu_ctx, case), fresh_decoder(gpu_ctx, case)
    fi, _ = new.reencode_as_inter(hdr, target, quality=case["quality"], records=False)
    fi_twin, _, _ = twin.reencode_as_inter(hdr, target, quality=case["quality"], records=True, append=True)
    got, got_twin = gpu_ctx.lf_search_decode([new, twin], [fi, fi_twin], [target, target])
    assert got == got_twin == searched(gpu_ctx, name)["result"]
    assert snapshot(new, fi) == snapshot(twin, fi_twin)
    # ... and it is the reference's frame
    _, mb, blocks = new.read_records(fi)
    msg = compare_records("%s frame 0" % name, mb, blocks, want_mb, rm.dense(want_mb, want_blocks))
    assert msg is None, msg
    for f in ("u", "lf_level", "segment_id", "coeff_index"):
        assert (mb[f] == want_mb[f]).all(), "%s frame 0: %s differs from the reference's" % (name, f)
    assert hashlib.sha256(new.raster_bytes(fi)).hexdigest() == case["sha256"][0]


# ---- 5. measure 1 ----
@pytest.mark.parametrize("name", rmm.CASES)
def test_sse_measure_finds_level_0_on_the_fixtures_the_stub_wrote(gpu_ctx, name):
    case = rmm.load_case(name)
    hdr, mb, blocks = rmm.parsed(name, "rebased")[0]
    assert hdr["loop_filter_level"] == 0
    d, plain = fresh_decoder(gpu_ctx, case), fresh_decoder(gpu_ctx, case)
    fi = append_wrong(d, name, parsed=lambda n: rmm.parsed(n, "rebased"))
    best, score, evaluated = d.lf_search_decode(fi, device_target(gpu_ctx, case["targets"][0]), measure="sse")
    assert (best, evaluated) == (0, 2)
    plain.decode_frame(plain.append_records(hdr, mb, blocks))          # (level 0: the unfiltered reconstruction)
    diff = plain.raster(0)[0].astype(np.int64) - case["targets"][0][0].astype(np.int64)
    assert score == lm.sse_score(int((diff * diff).sum()), case["pw"], case["ph"])
    assert d.raster_bytes(fi) == plain.raster_bytes(0) and hashlib.sha256(d.raster_bytes(fi)).hexdigest() == case["sha256"][0]


@pytest.mark.parametrize("name", lm.CASES)
def test_sse_measure_follows_the_rule_on_the_oracle_s_table(gpu_ctx, name):
    case = lm.load_case(name)
    d = fresh_decoder(gpu_ctx, case)
    fi = append_wrong(d, name)
    got = d.lf_search_decode(fi, device_target(gpu_ctx, case["targets"][0]), measure="sse")
    assert got == lm.rule(lm.sse_table(name), 0, 63)


# ---- 6. the whole chunk with nothing but bytes coming down ----
@pytest.mark.parametrize("name", lm.CASES)
def test_chain_writes_the_reference_s_bytes(gpu_ctx, name):
    case = lm.load_case(name)
    pred = walk(("pred", "lf_search", name), case["w"], case["h"], case["pred"])
    ref = walk(("rebased", "lf_search", name), case["w"], case["h"], case["rebased"], rm.decoder_state(case))
    d = fresh_decoder(gpu_ctx, case)
    for k, (hdr, ext, _, _, mb, blocks, _) in enumerate(ref):
        target = device_target(gpu_ctx, case["targets"][k])
        ext = cleared(ext, mb)
        if k == 0:
            fi, _ = d.reencode_as_inter(dict(hdr, loop_filter_level=63), target, quality=case["quality"], records=False)
            best, _, _ = d.lf_search_decode(fi, target)
            assert best == lm.REFERENCE[name][0]
            hdr, ext, sub_modes = dict(hdr, loop_filter_level=best, filter_adjustments_enabled=1), aa.with_zero_lf_deltas(ext), None
        else:
            fi, _ = d.rebase(hdr, pred[k][4], target, records=False)
            sub_modes = pred[k][2]
        data = d.serialize_frame(fi, hdr, ext, advance_state=True, sub_modes=sub_modes, optimise=True)
        want = case["rebased"][k]
        assert data == want, "%s frame %d: %d bytes, the reference wrote %d; first difference at byte %d" % (
            name, k, len(data), len(want), next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), min(len(data), len(want))))
        if k:
            d.decode_frame(fi)
        assert hashlib.sha256(d.raster_bytes(fi)).hexdigest() == case["sha256"][k]


# ---- 7. the stream goes on; rewind and release ----
def test_the_stream_goes_on_rewinds_and_releases(gpu_ctx):
    name = "ssim_best_80x80"
    case = lm.load_case(name)
    d = aa.Decoder(gpu_ctx, case["w"], case["h"])          # (references that are frames of its own: a rewind needs their rasters held)
    for fr in case["c0"]:
        d.get_frame_output(fr)
    first = d.frame_count()
    fi = append_wrong(d, name)
    assert fi == first
    assert d.lf_search_decode(fi, device_target(gpu_ctx, case["targets"][0])) == searched(gpu_ctx, name)["result"]
    hdr1, mb1, blocks1 = lm.parsed(name)[1]
    fi1 = d.append_records(hdr1, mb1, blocks1)
    d.decode_frame(fi1)
    rasters = [d.raster_bytes(fi), d.raster_bytes(fi1)]
    assert [hashlib.sha256(r).hexdigest() for r in rasters] == case["sha256"][:2]
    d.rewind_to(fi)
    d.decode_frame(fi); d.decode_frame(fi1)
    assert [d.raster_bytes(fi), d.raster_bytes(fi1)] == rasters, "after rewind_to the searched frame the stream decodes differently"
    with pytest.raises(aa.AlfalfaError):                   # a decoded frame is not searched again
        d.lf_search_decode(fi, device_target(gpu_ctx, case["targets"][0]))
    d.release_frame(fi)
    with pytest.raises(aa.AlfalfaError) as e:
        d.read_records(fi)
    assert "released" in e.value.message
    assert d.raster_bytes(fi1) == rasters[1]


# ---- 8. refusals ----
def test_refusals_leave_every_stream_as_it_was(gpu_ctx):
    name = "ssim_best_40x24"
    case = lm.load_case(name)
    target = device_target(gpu_ctx, case["targets"][0])
    L = capi.lib()

    def pending():
        d = fresh_decoder(gpu_ctx, case)
        return d, append_wrong(d, name)

    good, good_fi = pending()
    other, other_fi = pending()

    def job(dec, fi, **kw):
        j = capi.LfSearchJob()
        j.stream, j.frame_index, j.level_lo, j.level_hi = dec.h, fi, 0, 63
        j.original.y, j.original.u, j.original.v = (t.data_ptr() for t in target)
        j.original.y_stride, j.original.uv_stride = case["pw"], case["pw"] // 2
        j.best_level, j.evaluated, j.best_score = -5, -6, -7.0
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(code, text, second, measure=0, n=2, ctx=None, decs=()):
        jobs = (capi.LfSearchJob * 2)(job(good, good_fi), second)
        watched = [good, other] + list(decs)
        before = [d.frame_count() for d in watched]
        rc = L.aa_lf_search_decode_batch((ctx or gpu_ctx).h, jobs, n, measure)
        message = L.aa_last_error().decode()
        assert rc == code and message.startswith("aa_lf_search_decode_batch:") and text in message, (rc, message)
        assert [d.frame_count() for d in watched] == before
        # `next` is where it was: the pending frame is still each stream's next to decode -- a rewind to the frame behind it is refused
        # for a frame "not decoded yet" (and changes nothing), one to the frame itself is allowed
        for d, fi in ((good, good_fi), (other, other_fi)):
            assert L.aa_stream_rewind_to(d.h, fi + 1) == LOGIC and b"not been decoded" in L.aa_last_error(), "a refused call advanced a stream"
            assert L.aa_stream_rewind_to(d.h, fi) == 0
        for j in jobs:
            assert (j.best_level, j.evaluated, j.best_score) == (-5, -6, -7.0), "a refused call wrote an output field"

    ARG, LOGIC, UNSUPPORTED = -7, -3, -2
    refused(ARG, "null pointer", job(other, other_fi, stream=None))
    no_plane = job(other, other_fi)
    no_plane.original.y = None
    refused(ARG, "null pointer", no_plane)
    refused(ARG, "negative", job(other, other_fi), n=-1)
    assert L.aa_lf_search_decode_batch(gpu_ctx.h, None, 1, 0) == ARG and L.aa_lf_search_decode_batch(None, None, 0, 0) == ARG
    for lo, hi in ((-1, 5), (3, 64), (7, 6)):
        refused(ARG, "levels", job(other, other_fi, level_lo=lo, level_hi=hi))
    refused(ARG, "measure", job(other, other_fi), measure=2)
    foreign_ctx = aa.Context(gpu_ctx.device)
    foreign = fresh_decoder(foreign_ctx, case)
    refused(ARG, "another context", job(foreign, append_wrong(foreign, name)), decs=[foreign])
    del foreign, foreign_ctx
    refused(ARG, "also job 0", job(good, good_fi))
    key = aa.Decoder(gpu_ctx, case["w"], case["h"])
    key_fi, _ = key.parse_frame(case["c0"][0])
    refused(ARG, "key frame", job(key, key_fi), decs=[key])
    refused(ARG, "out of range", job(other, other_fi + 1))
    two = fresh_decoder(gpu_ctx, case)
    append_wrong(two, name)
    refused(LOGIC, "next to decode", job(two, append_wrong(two, name)), decs=[two])
    done = searched(gpu_ctx, name)
    refused(LOGIC, "next to decode", job(done["decoder"], done["fi"]), decs=[done["decoder"]])
    gone, gone_fi = pending()
    gone.release_frame(gone_fi)
    refused(LOGIC, "released", job(gone, gone_fi))
    try:
        gpu_ctx.set_schedule("diagonal")
        refused(UNSUPPORTED, "diagonal schedule", job(other, other_fi))
    finally:
        gpu_ctx.set_schedule("rows")
    with pytest.raises(ValueError):
        gpu_ctx.lf_search_decode([good], [good_fi], [target], measure="psnr")
    for levels, per_slice in ((0, 0), (9, 0), (4, -1)):
        with pytest.raises(aa.AlfalfaError):
            gpu_ctx.set_lf_search_round(levels, per_slice)
    assert gpu_ctx.lf_search_decode([], [], []) == []                 # n == 0 is AA_OK
    # ... and the same two decoders are still good for a call that is
    jobs = (capi.LfSearchJob * 2)(job(good, good_fi), job(other, other_fi))
    assert L.aa_lf_search_decode_batch(gpu_ctx.h, jobs, 2, 0) == 0, L.aa_last_error()
    for j, d, fi in ((jobs[0], good, good_fi), (jobs[1], other, other_fi)):
        assert (j.best_level, j.best_score, j.evaluated) == done["result"]
        assert snapshot(d, fi) == done["snap"]
