"""The re-encode on the GPU (aa_reencode_batch / Context.reencode_as_inter; needs a real MI355X) against the reference's xc-enc -r, bit
for bit, on the fixtures of tests/golden/reencode (tests/golden/make_reencode_golden.py; their census: tests/test_reencode_fixtures.py;
the same comparison on the host: tests/test_reencode_sim.py).

Per case: c0.state into a decoder, the new frame's header (quantiser factors, loop filter, refresh flags) from the product's parse of
rebased.ivf after c0.state, the edge-extended target uploaded; frame 0 by reencode_as_inter, frames 1.. by the rebase, each decoded.
Every macroblock: the 25 x 16 coefficients equal the parse of rebased.ivf, modes / references / vectors / b_modes / uv_mode / lf_level
and the five flags are equal, and the decoded padded planes hash to reencode_golden.json.  A difference is reported by macroblock,
class and block index."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import alfalfa_amd as aa
import rebase_model as rm
import reencode_model as rmm
from alfalfa_amd import capi
from test_gpu_rebase import compare_records, device_target

pytestmark = pytest.mark.gpu


def fresh_decoder(ctx, case):
    d = aa.Decoder(ctx, case["w"], case["h"])
    d.deserialize(case["state"])
    return d


_want = {}


def wanted(name):
    """-> [(header, mb, dense coefficients)] of rebased.ivf: made once."""
    if name not in _want:
        _want[name] = [(hdr, mb, rm.dense(mb, blocks)) for hdr, mb, blocks in rmm.parsed(name, "rebased")]
    return _want[name]


def check_frame0(name, got_mb, got_blocks):
    hdr, want_mb, want_dense = wanted(name)[0]
    msg = compare_records("%s frame 0" % name, got_mb, got_blocks, want_mb, want_dense)
    assert msg is None, msg
    # what compare_records leaves out: the sub-block modes of EVERY intra macroblock, the loop-filter level, the segment
    for f in ("u", "lf_level", "segment_id", "coeff_index"):
        bad = np.argwhere(np.array([[(got_mb[r, c][f] != want_mb[r, c][f]).any() for c in range(want_mb.shape[1])] for r in range(want_mb.shape[0])]))
        assert len(bad) == 0, "%s frame 0: %s differs from the reference's at macroblocks (row, column) %s" % (name, f, bad[:6].tolist())


def reencode_frame0(ctx, names, append=True):
    """Frame 0 of every case of `names` in ONE call, each on a fresh decoder -> [(decoder, frame_index, mb, blocks)]"""
    cases = [rmm.load_case(n) for n in names]
    decs = [fresh_decoder(ctx, c) for c in cases]
    targets = [device_target(ctx, c["targets"][0]) for c in cases]
    results = ctx.reencode_as_inter(decs, [wanted(n)[0][0] for n in names], targets, quality=[c["quality"] for c in cases], append=append)
    return [(d, fi, mb, blocks) for d, (fi, mb, blocks) in zip(decs, results)]


_single = {}


def single(ctx, name):
    """A case's frame 0 alone, checked against the reference and decoded -> (mb, blocks, raster); once per context."""
    key = (id(ctx), name)
    if key not in _single:
        (d, fi, mb, blocks), = reencode_frame0(ctx, [name])
        check_frame0(name, mb, blocks)
        assert fi == 0 and d.frame_count() == 1
        d.decode_frame(fi)
        raster = d.raster_bytes(fi)
        assert hashlib.sha256(raster).hexdigest() == rmm.load_case(name)["sha256"][0], "%s frame 0: records equal the reference's, the decoded planes do not hash to the golden" % name
        _single[key] = (mb, blocks, raster)
    return _single[key]


@pytest.mark.parametrize("name", rmm.CASES)
def test_reencode_equals_the_reference(gpu_ctx, name):
    single(gpu_ctx, name)


def test_one_call_for_all_fixtures_and_capped_rounds_equal_the_single_runs(gpu_ctx):
    """Mixed sizes and both qualities in one call; then with a round of the kernel capped at one and at two macroblocks, so that the
    anti-diagonals of the 5 x 5 frames (up to three macroblocks) take several rounds."""
    want = [single(gpu_ctx, n) for n in rmm.CASES]
    try:
        for slots in (16, 1, 2):
            gpu_ctx.set_reencode_slots(slots)
            for n, (d, fi, mb, blocks), (wmb, wblocks, wraster) in zip(rmm.CASES, reencode_frame0(gpu_ctx, rmm.CASES), want):
                assert (mb == wmb).all() and (blocks == wblocks).all(), "%d macroblocks per round, all fixtures in one call: %s differs from its single run" % (slots, n)
                d.decode_frame(fi)
                assert d.raster_bytes(fi) == wraster, "%d macroblocks per round: %s decodes differently" % (slots, n)
    finally:
        gpu_ctx.set_reencode_slots(16)
    with pytest.raises(aa.AlfalfaError):
        gpu_ctx.set_reencode_slots(0)


def test_the_cap_is_read_from_the_environment_at_context_creation(monkeypatch):
    monkeypatch.setenv("ALFALFA_AMD_REENC_SLOTS", "1")
    ctx = aa.Context(0)
    (d, fi, mb, blocks), = reencode_frame0(ctx, ["best_72x40"])
    check_frame0("best_72x40", mb, blocks)


@pytest.mark.parametrize("name", ["best_80x80", "rt_72x40"])
def test_the_whole_chunk(gpu_ctx, name):
    """xc-enc -r end to end: frame 0 by reencode_as_inter, frames 1.. by the rebase from pred.ivf's records, each decoded in turn."""
    case, pred, want = rmm.load_case(name), rmm.parsed(name, "pred"), wanted(name)
    d = fresh_decoder(gpu_ctx, case)
    for k, (hdr, want_mb, want_dense) in enumerate(want):
        target = device_target(gpu_ctx, case["targets"][k])
        if k == 0:
            fi, mb, blocks = d.reencode_as_inter(hdr, target, quality=case["quality"])
        else:
            fi, mb, blocks = d.rebase(hdr, pred[k][1], target)
        msg = compare_records("%s frame %d" % (name, k), mb, blocks, want_mb, want_dense)
        assert msg is None, msg
        d.decode_frame(fi)
        assert hashlib.sha256(d.raster_bytes(fi)).hexdigest() == case["sha256"][k], "%s frame %d: the decoded planes do not hash to the golden" % (name, k)


def test_without_append_nothing_is_appended_and_the_records_are_the_same(gpu_ctx):
    for name in ("best_72x40", "rt_80x80"):
        wmb, wblocks, wraster = single(gpu_ctx, name)
        (d, fi, mb, blocks), = reencode_frame0(gpu_ctx, [name], append=False)
        assert fi == -1 and d.frame_count() == 0, "append=False appended a frame"
        assert (mb == wmb).all() and (blocks == wblocks).all(), name
        # ... and they decode the same on a second decoder, once the caller appends them
        second = fresh_decoder(gpu_ctx, rmm.load_case(name))
        fi2 = second.append_records(dict(wanted(name)[0][0]), mb, blocks)
        second.decode_frame(fi2)
        assert second.raster_bytes(fi2) == wraster, "%s: append_records of the returned records decodes differently" % name


def test_refusals_leave_every_stream_as_it_was(gpu_ctx):
    name = "best_16x16"
    case = rmm.load_case(name)
    hdr = dict(wanted(name)[0][0])
    target = device_target(gpu_ctx, case["targets"][0])
    good, other = fresh_decoder(gpu_ctx, case), fresh_decoder(gpu_ctx, case)

    def refused(kind, text, decs, hdrs, targets):
        before = [d.frame_count() for d in decs]
        with pytest.raises(aa.AlfalfaError) as e:
            gpu_ctx.reencode_as_inter(decs, hdrs, targets)
        assert e.value.kind == kind and "aa_reencode_batch" in e.value.message and text in e.value.message, e.value
        assert [d.frame_count() for d in decs] == before, "a refused call appended a frame"

    # (the good job comes first in every call: it must not be appended either)
    refused("BadArgument", "key frame", [good, other], [hdr, dict(hdr, key_frame=1)], [target, target])
    refused("Unsupported", "segmentation", [good, other], [hdr, dict(hdr, segmentation_enabled=1)], [target, target])
    big = rmm.load_case("best_72x40")
    refused("BadArgument", "dimensions", [good, fresh_decoder(gpu_ctx, big)], [hdr, hdr], [target, device_target(gpu_ctx, big["targets"][0])])
    refused("BadArgument", "also job 0", [good, good], [hdr, hdr], [target, target])
    pending = fresh_decoder(gpu_ctx, case)
    w = rmm.parsed(name, "rebased")[0]
    pending.append_records(dict(w[0]), w[1], w[2])
    refused("LogicError", "not decoded", [good, pending], [hdr, hdr], [target, target])

    # the C call itself: null pointers, a quality that is none, and a coefficient array that is too small (the message names the count needed)
    L = capi.lib()
    h = gpu_ctx._header_struct(hdr)
    nmb = hdr["mb_width"] * hdr["mb_height"]
    out_mb = np.zeros(nmb, capi.MB_INFO_DTYPE)
    out_cf = np.zeros((25 * nmb, 16), np.int16)

    def job(dec, **kw):
        j = capi.ReencodeJob()
        j.stream, j.hdr = dec.h, C.pointer(h)
        j.target.y, j.target.u, j.target.v = (t.data_ptr() for t in target)
        j.target.y_stride, j.target.uv_stride = case["pw"], case["pw"] // 2
        j.quality, j.append = 0, 1
        j.mbs_out, j.coeffs_out, j.coeff_capacity_blocks = out_mb.ctypes.data_as(C.c_void_p), out_cf.ctypes.data_as(C.c_void_p), len(out_cf)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    for broken in (job(other, mbs_out=None), job(other, hdr=None), job(other, stream=None), job(other, coeffs_out=None)):
        jobs = (capi.ReencodeJob * 2)(job(good), broken)
        assert L.aa_reencode_batch(gpu_ctx.h, jobs, 2) == -7 and b"null pointer" in L.aa_last_error(), L.aa_last_error()
    jobs = (capi.ReencodeJob * 2)(job(good), job(other, quality=2))
    assert L.aa_reencode_batch(gpu_ctx.h, jobs, 2) == -7 and b"quality" in L.aa_last_error(), L.aa_last_error()
    assert L.aa_reencode_batch(gpu_ctx.h, None, 1) == -7
    need = single(gpu_ctx, name)[1].shape[0]
    assert need > 1
    jobs = (capi.ReencodeJob * 2)(job(good), job(other, coeff_capacity_blocks=need - 1))
    assert L.aa_reencode_batch(gpu_ctx.h, jobs, 2) == -7
    assert b"too small" in L.aa_last_error() and (b"%d blocks needed" % need) in L.aa_last_error(), L.aa_last_error()
    assert good.frame_count() == 0 and other.frame_count() == 0
    # ... and the same two decoders are still good for a call that is
    out_mb2, out_cf2 = np.zeros_like(out_mb), np.zeros_like(out_cf)
    jobs = (capi.ReencodeJob * 2)(job(good), job(other, mbs_out=out_mb2.ctypes.data_as(C.c_void_p), coeffs_out=out_cf2.ctypes.data_as(C.c_void_p)))
    assert L.aa_reencode_batch(gpu_ctx.h, jobs, 2) == 0, L.aa_last_error()
    assert (jobs[0].frame_index, jobs[1].frame_index, jobs[1].num_coeff_blocks) == (0, 0, need)
    assert (out_mb == out_mb2).all() and (out_cf == out_cf2).all()
    timing = gpu_ctx.reencode_timing()
    assert timing["call_ms"] > 0 and timing["kernels_ms"] > 0
