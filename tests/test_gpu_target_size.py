"""The frame-size estimate and the target-size quantiser search on the GPU (aa_estimate_size_batch / aa_target_size_batch;
Context.estimate_frame_sizes / Context.target_size_q; needs a real MI355X) against the reference's xc-enc -y QI (every printed
[estimated size=N]) and xc-enc -F (every chosen quantiser index) on the fixtures of tests/golden/target_size, and against the host model
(tests/cpp/estimate_sim.cc) where the reference gives no number: the sizes of the candidates a search visits, and a picture of another size.
Which frames are compared with the reference is decided on the host (tests/test_estimate_sim.py); every frame is compared with the host
model.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import alfalfa_amd as aa
import estimate_model as em
import make_y4m
from alfalfa_amd import capi
from test_estimate_sim import f_run, y_run
from test_gpu_rebase import device_target

pytestmark = pytest.mark.gpu


def decoder_before(ctx, name, k):
    """A decoder that has decoded the fixture's own frames 0 .. k-1"""
    case = em.CASES[name]
    d = aa.Decoder(ctx, case["width"], case["height"])
    for fr in em.frames(name)[:k]:
        d.parse_and_decode_frame(fr["bytes"])
    return d


def y_jobs(name):
    """The four estimates of a -y fixture as independent jobs -> [(k, frame, carry in front of it, size and carry the host model gives)]"""
    run, carry, out = y_run(name), em.INITIAL_CARRY, []
    for k, fr in enumerate(em.frames(name)):
        before = carry if fr["key"] else em.carry_in_front_of(k, carry)
        out.append((k, fr, before, run[k]))
        if not fr["key"]:
            carry = run[k]["carry"]
    return out


# ---- 1. every fixture estimate, the carry handed on from frame to frame as the call returns it ----
@pytest.mark.parametrize("name", em.Y_CASES)
def test_every_estimate_equals_the_reference(gpu_ctx, name):
    case = em.CASES[name]
    run, carry, compared = y_run(name), em.INITIAL_CARRY, 0
    for k, fr in enumerate(em.frames(name)):
        d = decoder_before(gpu_ctx, name, k)
        before = carry if fr["key"] else em.carry_in_front_of(k, carry)
        size, after = d.estimate_frame_size(device_target(gpu_ctx, fr["target"]), case["q_index"], key_frame=fr["key"], quality=case["quality"], carry=before)
        print("%s frame %d: %d, host model %d, reference %d%s" % (name, k, size, run[k]["size"], case["estimates"][k], "" if run[k]["comparable"] else " (not compared)"))
        assert size == run[k]["size"], "%s frame %d: %d, the host model gives %d" % (name, k, size, run[k]["size"])
        if fr["key"]:
            assert after == before, "a key estimate changed the carry"
        else:
            assert after[:3] == run[k]["carry"][:3] and after[3] == before[3], "%s frame %d: carry %s, the host model gives %s" % (name, k, after, run[k]["carry"])
            carry = after
        if run[k]["comparable"]:
            compared += 1
            assert size == case["estimates"][k], "%s frame %d: %d, the reference prints %d" % (name, k, size, case["estimates"][k])
    assert compared >= 2


# ---- 2. every -F frame: the choice, the number of estimates, the visited candidates ----
@pytest.mark.parametrize("name", em.F_CASES)
def test_every_chosen_quantiser_equals_the_reference(gpu_ctx, name):
    case = em.CASES[name]
    for k, (fr, want) in enumerate(zip(em.frames(name), f_run(name))):
        d = decoder_before(gpu_ctx, name, k)
        lo, hi = want["range"]
        q, visited, after = d.target_size_q(device_target(gpu_ctx, fr["target"]), case["targets"][k], lo, hi, key_frame=fr["key"], quality=case["quality"], carry=want["carry_before"])
        print("%s frame %d: chose %d in %d..%d after %s, reference %d" % (name, k, q, lo, hi, visited, case["chosen_q"][k]))
        assert (q, visited) == (want["q"], want["visited"]), "%s frame %d: %d after %s, the host model gives %d after %s" % (name, k, q, visited, want["q"], want["visited"])
        assert after[:3] == want["carry"][:3]
        if want["comparable"]:
            assert q == case["chosen_q"][k], "%s frame %d: chose %d, the reference chose %d" % (name, k, q, case["chosen_q"][k])
        assert gpu_ctx.target_size_timing()["rounds"] == len(visited)


# ---- 3. all fixture jobs in one call; capped rounds; one job per slice ----
def all_in_one_call(ctx, names):
    jobs = [(name, j) for name in names for j in y_jobs(name)]
    decs = [decoder_before(ctx, name, k) for name, (k, _, _, _) in jobs]
    targets = [device_target(ctx, fr["target"]) for _, (_, fr, _, _) in jobs]
    got = ctx.estimate_frame_sizes(decs, targets, [em.CASES[name]["q_index"] for name, _ in jobs], key_frame=[fr["key"] for _, (_, fr, _, _) in jobs],
                                   quality=[em.CASES[name]["quality"] for name, _ in jobs], carry=[before for _, (_, _, before, _) in jobs])
    for (name, (k, fr, before, want)), (size, after) in zip(jobs, got):
        assert size == want["size"], "%s frame %d in one call with %d jobs: %d, alone %d" % (name, k, len(jobs), size, want["size"])
        assert after[:3] == (before[:3] if fr["key"] else want["carry"][:3])
    return len(jobs)


def test_all_fixture_estimates_in_one_call_equal_the_single_runs(gpu_ctx):
    assert all_in_one_call(gpu_ctx, em.Y_CASES) == 4 * len(em.Y_CASES) == 80


def test_capped_rounds_and_one_job_per_slice_give_the_same(gpu_ctx):
    """The 5 x 5 small frames (anti-diagonals of up to three macroblocks) at 16, 2 and 1 macroblocks per round, then every job in a
    slice of its own."""
    names = [n for n in em.Y_CASES if "272x272" in n]
    assert len(names) == 4
    try:
        for slots in (16, 2, 1):
            gpu_ctx.set_reencode_slots(slots)
            all_in_one_call(gpu_ctx, names)
        gpu_ctx.set_reencode_slots(16)
        gpu_ctx.set_target_size_round(1)
        all_in_one_call(gpu_ctx, names)
    finally:
        gpu_ctx.set_reencode_slots(16)
        gpu_ctx.set_target_size_round(0)


# ---- 4. a picture of another size against the host model ----
def test_560x288_equals_the_host_model(gpu_ctx):
    """A 9 x 5 small frame (140 x 72 pixels: partial macroblocks at both of its edges): key and inter estimates in both qualities, and one
    search of each kind, from the decoder's own reference."""
    w, h = 560, 288
    assert em.small_size(w, h) == (9, 5)
    pictures = em.originals(w, h, 5, "high", 2)
    d = aa.Decoder(gpu_ctx, w, h)
    template = next(iter(em.frames("y_80x80_best_q40")))["bytes"]
    hdr = dict(aa.Parser(80, 80).parse(template)[0], width=w, height=h, mb_width=35, mb_height=18, num_macroblocks=35 * 18, q_index=40, quant=[capi.quant_factors(40)] * 4,
               num_coeff_blocks=0, num_intra_mbs=0)
    key = {"key": True, "target": pictures[0], "ref": None, "probs_before": np.zeros(1101, np.uint8)}
    targets = [device_target(gpu_ctx, p) for p in pictures]
    for q in (6, 40):
        assert d.estimate_frame_size(targets[0], q, key_frame=True)[0] == em.sim_estimate(w, h, key, q, "best", em.INITIAL_CARRY)[0]
    fi = d.encode_frame(hdr, targets[0])[0]
    d.decode_frame(fi)
    # (appending records advances no DecoderState: the decoder's tables are still a new decoder's)
    inter = {"key": False, "target": pictures[1], "ref": [p.copy() for p in d.raster(fi)], "probs_before": np.array(aa.Parser(w, h).probs(), np.uint8).copy()}
    for quality in ("best", "rt"):
        for q, carry in ((6, (0, 0, 0, 0)), (40, (7, 9, 11, 1))):
            got = d.estimate_frame_size(targets[1], q, quality=quality, carry=carry)
            want = em.sim_estimate(w, h, inter, q, quality, carry)
            assert got == want, (quality, q, got, want)
        goal = em.sim_estimate(w, h, inter, 40, quality, (0, 0, 0, 1))[0]           # (the size at index 40: the choice lies inside the range)
        got = d.target_size_q(targets[1], goal, 4, 127, quality=quality, carry=(0, 0, 0, 1))
        want = em.sim_target(w, h, inter, quality, (0, 0, 0, 1), 4, 127, goal)
        assert got == want and 4 < got[0] < 127 and len(got[1]) >= 6, (quality, got, want)
    goal = em.sim_estimate(w, h, key, 40, "best", em.INITIAL_CARRY)[0]
    got = d.target_size_q(targets[0], goal, 4, 127, key_frame=True)
    want = em.sim_target(w, h, key, "best", em.INITIAL_CARRY, 4, 127, goal)
    assert got == want and 4 < got[0] < 127 and len(got[1]) >= 6, (got, want)


# ---- 5. nothing changes ----
def test_streams_are_unchanged_afterwards(gpu_ctx):
    name = "y_80x80_rt_q40"
    case = em.CASES[name]
    frs = em.frames(name)
    decs = [decoder_before(gpu_ctx, name, k) for k in (1, 2, 3)]
    counts, hashes = [d.frame_count() for d in decs], gpu_ctx.decoder_hashes(decs)
    targets = [device_target(gpu_ctx, frs[k]["target"]) for k in (1, 2, 3)]
    gpu_ctx.estimate_frame_sizes(decs, targets, 40, quality="rt")
    gpu_ctx.target_size_q(decs, targets, [2000, 3000, 100], quality="rt")
    gpu_ctx.estimate_frame_sizes(decs, targets, 40, key_frame=True)
    assert [d.frame_count() for d in decs] == counts and gpu_ctx.decoder_hashes(decs) == hashes
    # ... and the decoders go on decoding their streams
    for d, k in zip(decs, (1, 2, 3)):
        d.parse_and_decode_frame(frs[k]["bytes"])
    assert case["quality"] == "rt"


# ---- 6. refusals ----
def test_refusals_change_nothing(gpu_ctx):
    name = "y_16x16_best_q40"
    frs = em.frames(name)
    target = device_target(gpu_ctx, frs[1]["target"])
    good, other, fresh = decoder_before(gpu_ctx, name, 1), decoder_before(gpu_ctx, name, 1), aa.Decoder(gpu_ctx, 16, 16)
    foreign_ctx = aa.Context(0)
    foreign = aa.Decoder(foreign_ctx, 16, 16)

    def refused(kind, text, call, who, *args, **kw):
        with pytest.raises(aa.AlfalfaError) as e:
            call(*args, **kw)
        assert e.value.kind == kind and e.value.message.startswith(who + ":") and text in e.value.message, e.value

    for who, call, extra in (("aa_estimate_size_batch", gpu_ctx.estimate_frame_sizes, ([40, 40],)), ("aa_target_size_batch", gpu_ctx.target_size_q, ([1000, 1000],))):
        refused("BadArgument", "also job 0", call, who, [good, good], [target, target], *extra)
        refused("BadArgument", "another context", call, who, [good, foreign], [target, target], *extra)
        refused("LogicError", "not a decoded or imported raster", call, who, [good, fresh], [target, target], *extra)
        assert call([good, fresh], [target, target], *extra, key_frame=[False, True])          # (a key job needs nothing before it)
    refused("BadArgument", "q_index", gpu_ctx.estimate_frame_sizes, "aa_estimate_size_batch", [good, other], [target, target], [40, 128])
    refused("BadArgument", "q_index", gpu_ctx.estimate_frame_sizes, "aa_estimate_size_batch", [good, other], [target, target], [40, -1])
    refused("BadArgument", "outside 0..127", gpu_ctx.target_size_q, "aa_target_size_batch", [good, other], [target, target], [1000, 1000], q_lo=[4, -1])
    refused("BadArgument", "outside 0..127", gpu_ctx.target_size_q, "aa_target_size_batch", [good, other], [target, target], [1000, 1000], q_hi=[127, 128])
    refused("BadArgument", "q_lo > q_hi", gpu_ctx.target_size_q, "aa_target_size_batch", [good, other], [target, target], [1000, 1000], q_lo=[4, 60], q_hi=[127, 59])
    tiny = aa.Decoder(gpu_ctx, 3, 16)
    tiny_target = device_target(gpu_ctx, em.pad(next(make_y4m.synth_frames(3, 16, 1, 1, "low")), 16, 16))
    refused("Unsupported", "under 4", gpu_ctx.estimate_frame_sizes, "aa_estimate_size_batch", [good, tiny], [target, tiny_target], [40, 40], key_frame=True)
    pending = decoder_before(gpu_ctx, name, 1)
    hdr = aa.Parser(16, 16).parse(frs[0]["bytes"])[0]
    pending.encode_frame(hdr, target)
    refused("LogicError", "not decoded", gpu_ctx.estimate_frame_sizes, "aa_estimate_size_batch", [good, pending], [target, target], [40, 40])

    # the C calls themselves: null pointers, a quality that is none, n < 0, n == 0; no output field of a refused call is written
    L = capi.lib()

    def job(kind, dec, **kw):
        j = kind()
        j.stream = dec.h
        j.target.y, j.target.u, j.target.v = (t.data_ptr() for t in target)
        j.target.y_stride, j.target.uv_stride = 16, 8
        j.key_frame, j.quality = 0, 0
        if kind is capi.EstimateSizeJob:
            j.q_index, j.size_out = 40, 12345
        else:
            j.q_lo, j.q_hi, j.target_size, j.q_index, j.estimates = 4, 127, 1000, -5, -5
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    for kind, call, who in ((capi.EstimateSizeJob, L.aa_estimate_size_batch, b"aa_estimate_size_batch"), (capi.TargetSizeJob, L.aa_target_size_batch, b"aa_target_size_batch")):
        for broken in (job(kind, other, stream=None), job(kind, other, quality=2)):
            jobs = (kind * 2)(job(kind, good), broken)
            assert call(gpu_ctx.h, jobs, 2) == -7 and L.aa_last_error().startswith(who + b": job 1:"), L.aa_last_error()
            assert jobs[0].size_out == 12345 if kind is capi.EstimateSizeJob else (jobs[0].q_index, jobs[0].estimates) == (-5, -5)
        broken = job(kind, other)
        broken.target.u = None
        jobs = (kind * 2)(job(kind, good), broken)
        assert call(gpu_ctx.h, jobs, 2) == -7 and b"null pointer" in L.aa_last_error()
        assert call(gpu_ctx.h, None, 1) == -7 and call(gpu_ctx.h, jobs, -1) == -7
        assert call(gpu_ctx.h, jobs, 0) == 0 and call(gpu_ctx.h, None, 0) == 0
    assert good.frame_count() == 1 and other.frame_count() == 1
    # ... and the same decoders are still good for a call that is
    assert gpu_ctx.estimate_frame_sizes([good, other], [target, target], 40)[0][0] == em.CASES[name]["estimates"][1]
    timing = gpu_ctx.target_size_timing()
    assert timing["call_ms"] > 0 and timing["decisions_ms"] > 0 and timing["rounds"] == 1


# ---- 7. end to end ----
def test_end_to_end_search_encode_serialise_parse_back(gpu_ctx):
    """target_size_q -> encode_frames at the chosen index -> serialize_frames( optimise=True ) -> the product's parser reads the records
    back; the choices are the reference's, under real-time quality with the range around the last frame's index."""
    name = "f_80x80_rt"
    case = em.CASES[name]
    w, h = case["width"], case["height"]
    d = aa.Decoder(gpu_ctx, w, h)
    ref_parser, p = aa.Parser(w, h), aa.Parser(w, h)
    carry, last_q = aa.estimate_carry(), None
    for k, (fr, want) in enumerate(zip(em.frames(name), f_run(name))):
        fixture_hdr = ref_parser.parse(fr["bytes"])[0]
        ext = ref_parser.header_ext()
        target = device_target(gpu_ctx, fr["target"])
        lo, hi = aa.target_size_range(last_q)
        before = carry if fr["key"] else em.carry_in_front_of(k, carry)
        q, visited, after = d.target_size_q(target, case["targets"][k], lo, hi, key_frame=fr["key"], quality="rt", carry=before)
        if not fr["key"]:
            carry = after
        assert q == case["chosen_q"][k] and (lo, hi) == want["range"]
        hdr = dict(fixture_hdr, q_index=q, quant=[capi.quant_factors(q)] * 4, num_coeff_blocks=0, num_intra_mbs=0)
        fi, mb, blocks = d.encode_frame(hdr, target, quality="rt")
        held = d.frame_header(fi)
        data = d.serialize_frame(fi, held, ext, advance_state=True, optimise=True)
        phdr, pmb, pblocks = p.parse(data)
        assert phdr["q_index"] == q and phdr["key_frame"] == int(fr["key"])
        for f in ("y_mode", "uv_mode", "ref_frame", "nz_mask", "flags", "coeff_index"):
            assert (pmb[f] == mb[f]).all(), (k, f)
        assert (pmb["u"] == mb["u"]).all() and pblocks.tobytes() == blocks.tobytes()
        d.decode_frame(fi)
        last_q = q
