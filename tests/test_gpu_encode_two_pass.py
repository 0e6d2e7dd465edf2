"""The forward encoder's key frames in the reference's TWO passes on the GPU (aa_encode_two_pass_batch / Context.encode_frames(
two_pass=True ); needs a real MI355X) against xc-enc -i y4m -y QI -q best|rt --two-pass, bit for bit, on the fixtures of
tests/golden/two_pass and tests/golden/two_pass_crafted (tests/two_pass_model.py; the same comparison on the host:
tests/test_encode2_sim.py; the sweep over more crafted pictures: tests/test_gpu_encode_two_pass_crafted.py).

The header of each new frame is the product's parse of the fixture frame (quantiser, loop-filter level, refresh flags); every macroblock's
modes, b_modes, flags, nz_mask, coeff_index, lf_level and all 25 x 16 coefficients must equal the parse of the fixture frame, the decoded
planes what the fixture's bytes decode to, the written header's token_prob_update the fixture's, and the serialised frame the fixture's
bytes.  All comparisons are exact."""
import numpy as np
import pytest

import alfalfa_amd as aa
import encode_model as em
import make_y4m
import two_pass_model as tp
from test_gpu_encode import check_records, decoder_before, single
from test_gpu_rebase import device_target

pytestmark = pytest.mark.gpu


def first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


_single2 = {}


def single2(ctx, name):
    """One fixture case alone: the key frame in two passes, checked against the reference, serialised with the first pass's updates,
    decoded; then the inter frame behind it from the decoder's own decode -> (key: mb, blocks, updates, raster, bytes; inter: mb, blocks,
    bytes); once per context."""
    key = (id(ctx), name)
    if key not in _single2:
        c = tp.case(name)
        k, i = c["frames"]
        d = aa.Decoder(ctx, c["w"], c["h"])
        fi, mb, blocks, updates = d.encode_frame(k["header"], device_target(ctx, k["target"]), quality=c["quality_name"], two_pass=True)
        check_records("%s key frame, two passes" % name, k, mb, blocks)
        assert fi == 0 and updates.shape == (2112,) and updates.dtype == np.uint8
        data, ext, _ = d.serialize_frame(fi, k["header"], k["ext"], advance_state=True, optimise=True, details=True, first_pass_updates=updates)
        written = np.concatenate([np.array(ext["token_prob_update"], np.uint8).reshape(-1), np.array(ext["token_prob"], np.uint8).reshape(-1)])
        wrong = np.flatnonzero(written != k["updates"])
        assert len(wrong) == 0, "%s: token_prob_update as written differs from the fixture's header at %s" % (name, wrong[:8].tolist())
        d.decode_frame(fi)
        raster = d.raster_bytes(fi)
        assert raster == b"".join(p.tobytes() for p in k["decoded"]), "%s: records equal the reference's, the decoded planes are not what the fixture's bytes decode to" % name
        # the inter frame behind it: single pass, from the decoder's own decode of the two-pass key frame
        fi1, mb1, blocks1 = d.encode_frame(i["header"], device_target(ctx, i["target"]), quality=c["quality_name"])
        check_records("%s inter frame behind the two-pass key frame" % name, i, mb1, blocks1)
        data1 = d.serialize_frame(fi1, i["header"], i["ext"], advance_state=True, optimise=True)
        d.decode_frame(fi1)
        assert d.raster_bytes(fi1) == b"".join(p.tobytes() for p in i["decoded"]), "%s: the inter frame decodes differently" % name
        _single2[key] = ((mb, blocks, updates, raster, data), (mb1, blocks1, data1))
    return _single2[key]


# ---- 1. records, coefficients, decoded planes, token_prob_update ----
@pytest.mark.parametrize("name", tp.CASES)
def test_two_pass_key_frame_equals_the_reference(gpu_ctx, name):
    single2(gpu_ctx, name)


# ---- 2. bytes ----
@pytest.mark.parametrize("name", tp.CASES)
def test_serialised_key_frame_is_the_fixture_s_bytes(gpu_ctx, name):
    data, want = single2(gpu_ctx, name)[0][4], tp.case(name)["frames"][0]["bytes"]
    assert data == want, "%s: %d bytes, the reference wrote %d; first difference at byte %d" % (name, len(data), len(want), first_difference(data, want))


def test_without_the_first_pass_s_updates_some_frame_is_not_the_fixture_s(gpu_ctx):
    """The merge is not a no-op: serialised without first_pass_updates, a fixture whose header keeps a first-pass field differs."""
    name = "80x80_q45"
    c = tp.case(name)
    k = c["frames"][0]
    d = aa.Decoder(gpu_ctx, c["w"], c["h"])
    fi, _, _, updates = d.encode_frame(k["header"], device_target(gpu_ctx, k["target"]), quality=c["quality_name"], two_pass=True)
    assert d.serialize_frame(fi, k["header"], k["ext"], optimise=True, first_pass_updates=updates) == k["bytes"]
    assert d.serialize_frame(fi, k["header"], k["ext"], optimise=True) != k["bytes"]
    assert d.serialize_frame(fi, k["header"], k["ext"], optimise=True, first_pass_updates=np.zeros(2112, np.uint8)) == d.serialize_frame(fi, k["header"], k["ext"], optimise=True)


# ---- 3. the inter frame behind the key frame ----
@pytest.mark.parametrize("name", tp.CASES)
def test_inter_frame_behind_the_two_pass_key_frame_is_the_fixture_s(gpu_ctx, name):
    data, want = single2(gpu_ctx, name)[1][2], tp.case(name)["frames"][1]["bytes"]
    assert data == want, "%s frame 1: %d bytes, the reference wrote %d; first difference at byte %d" % (name, len(data), len(want), first_difference(data, want))


# ---- 4. one call for everything; capped rounds ----
OTHERS = [("best_80x80", "pred", 0), ("rt_80x80", "c0", 0), ("best_72x40", "c0", 1), ("rt_low_80x80", "pred", 1), ("best_16x16", "c0", 2)]


def test_one_call_for_all_cases_mixed_with_single_pass_jobs_and_capped_rounds(gpu_ctx):
    """Every two-pass case, single-pass key jobs and inter jobs of tests/golden/reencode (one inter job with its flag set: it is ignored) in
    ONE call, at 16, 2 and 1 macroblocks per round: every job equals its single run."""
    want2 = [single2(gpu_ctx, name)[0] for name in tp.CASES]
    want1 = [single(gpu_ctx, *f) for f in OTHERS]
    try:
        for slots in (16, 2, 1):
            gpu_ctx.set_reencode_slots(slots)
            cases = [tp.case(name) for name in tp.CASES]
            frs = [em.frames(n, w)[k] for n, w, k in OTHERS]
            decs = [aa.Decoder(gpu_ctx, c["w"], c["h"]) for c in cases] + [decoder_before(gpu_ctx, n, w, k) for n, w, k in OTHERS]
            headers = [c["frames"][0]["header"] for c in cases] + [fr["header"] for fr in frs]
            targets = [device_target(gpu_ctx, c["frames"][0]["target"]) for c in cases] + [device_target(gpu_ctx, fr["target"]) for fr in frs]
            qualities = [c["quality_name"] for c in cases] + [fr["quality_name"] for fr in frs]
            flags = [True] * len(cases) + [False, False, False, True, False]
            # (interleaved, so that the call has to sort the kinds itself)
            order = sorted(range(len(decs)), key=lambda i: (i * 7) % len(decs))
            out = gpu_ctx.encode_frames([decs[i] for i in order], [headers[i] for i in order], [targets[i] for i in order], quality=[qualities[i] for i in order],
                                        two_pass=[flags[i] for i in order])
            got = dict(zip(order, out))
            for i, name in enumerate(tp.CASES):
                fi, mb, blocks, updates = got[i]
                wmb, wblocks, wupdates, wraster, _ = want2[i]
                assert (mb == wmb).all() and (blocks == wblocks).all() and (updates == wupdates).all(), "%d macroblocks per round: %s differs from its single run" % (slots, name)
                decs[i].decode_frame(fi)
                assert decs[i].raster_bytes(fi) == wraster, "%d macroblocks per round: %s decodes differently" % (slots, name)
            for i, f in enumerate(OTHERS):
                fi, mb, blocks, updates = got[len(cases) + i]
                wmb, wblocks, wraster = want1[i]
                assert (mb == wmb).all() and (blocks == wblocks).all() and not updates.any(), "%d macroblocks per round: the single-pass job %s differs from its single run" % (slots, f)
                decs[len(cases) + i].decode_frame(fi)
                assert decs[len(cases) + i].raster_bytes(fi) == wraster
    finally:
        gpu_ctx.set_reencode_slots(16)


# ---- 5. diagonals longer than the slots ----
def test_560x288_at_16_slots_at_1_slot_and_on_the_host(gpu_ctx):
    """35 x 18 macroblocks: anti-diagonals of up to 18 macroblocks, more than the 16 slots of a round, and 630 macroblocks over ten
    workgroups of the pass between the passes.  At 16 slots, at 1 slot and by the host simulation: records, blocks and the first pass's
    updates are byte-equal."""
    from test_encode2_sim import sim_lib, sim_two_pass
    w, h, q = 560, 288, 45
    planes = em.pad(next(iter(make_y4m.synth_frames(w, h, 1, 5, "high"))), w, h)
    hdr = em.header_like(tp.case("80x80_q45")["frames"][0]["header"], w, h, q, key=True)
    got = {}
    try:
        for slots in (16, 1):
            gpu_ctx.set_reencode_slots(slots)
            d = aa.Decoder(gpu_ctx, w, h)
            fi, mb, blocks, updates = d.encode_frame(hdr, device_target(gpu_ctx, planes), quality="best", two_pass=True)
            data, ext, _ = d.serialize_frame(fi, hdr, tp.case("80x80_q45")["frames"][0]["ext"], optimise=True, details=True, first_pass_updates=updates)
            d.decode_frame(fi)
            got[slots] = (mb, blocks, updates, d.raster_bytes(fi), ext)
    finally:
        gpu_ctx.set_reencode_slots(16)
    mb, blocks, updates, raster, ext = got[16]
    assert mb.shape == (18, 35)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got[16][:3], got[1][:3])) and raster == got[1][3], "16 slots and 1 slot differ"
    smb, sdense, srecon, _, supdates, _ = sim_two_pass(sim_lib(), hdr, planes)
    smb, sblocks = em.finished_records(smb, sdense, hdr["loop_filter_level"])
    assert mb.tobytes() == smb.tobytes() and blocks.tobytes() == sblocks.tobytes(), "the kernel and the host simulation differ"
    written = np.concatenate([np.array(ext["token_prob_update"], np.uint8).reshape(-1), np.array(ext["token_prob"], np.uint8).reshape(-1)])
    assert (written == supdates).all(), "token_prob_update after both passes: the kernels and the host simulation differ"
    assert raster == srecon.tobytes()              # (level 0: the decoded frame is the second pass's reconstruction)


# ---- 6. device-resident records ----
def test_records_kept_on_the_device_equal_the_host_record_call(gpu_ctx):
    names = ["72x40_q90", "80x80_q93", "272x272_q18", "80x80low_rt_q30", "dot_rt_q26"]      # (the last: B_PRED chosen after a 16x16 mode)
    cases = [tp.case(n) for n in names]
    twins = [[aa.Decoder(gpu_ctx, c["w"], c["h"]) for c in cases] for _ in range(2)]
    headers = [c["frames"][0]["header"] for c in cases]
    qualities = [c["quality_name"] for c in cases]
    host = gpu_ctx.encode_frames(twins[0], headers, [device_target(gpu_ctx, c["frames"][0]["target"]) for c in cases], quality=qualities, two_pass=True)
    dev = gpu_ctx.encode_frames(twins[1], headers, [device_target(gpu_ctx, c["frames"][0]["target"]) for c in cases], quality=qualities, two_pass=True, records=False)
    for name, c, (fi, mb, blocks, updates), (dfi, nblocks, dupdates), a, b in zip(names, cases, host, dev, twins[0], twins[1]):
        assert (fi, dfi) == (0, 0) and nblocks == len(blocks) and (updates == dupdates).all(), name
        _, rmb, rblocks = b.read_records(dfi)
        assert rmb.tobytes() == mb.tobytes() and rblocks.tobytes() == blocks.tobytes(), "%s: the records kept on the device differ from the host-record call's" % name
        k = c["frames"][0]
        assert b.serialize_frame(dfi, k["header"], k["ext"], optimise=True, first_pass_updates=dupdates) == k["bytes"], name
        a.decode_frame(fi); b.decode_frame(dfi)
        assert a.raster_bytes(fi) == b.raster_bytes(dfi), name


# ---- 7. the default ----
def test_without_the_flag_the_call_is_today_s(gpu_ctx):
    keys = [(n, "pred", 0) for n in em.CASES] + [(n, "c0", 0) for n in em.CASES]
    for f in keys:
        wmb, wblocks, _ = single(gpu_ctx, *f)
        fr = em.frames(*f[:2])[f[2]]
        for kw in ({}, {"two_pass": False}, {"two_pass": [False]}):
            d = decoder_before(gpu_ctx, *f)
            out = gpu_ctx.encode_frames([d], [fr["header"]], [device_target(gpu_ctx, fr["target"])], quality=fr["quality_name"], **kw)[0]
            assert len(out) == 3 and out[0] == 0 and out[1].tobytes() == wmb.tobytes() and out[2].tobytes() == wblocks.tobytes(), (f, kw)


# ---- 8. refusals ----
def test_refusals(gpu_ctx):
    c = tp.case("16x16_q93")
    k = c["frames"][0]
    d = aa.Decoder(gpu_ctx, c["w"], c["h"])
    target = device_target(gpu_ctx, k["target"])
    with pytest.raises(ValueError):
        d.encode_frame(k["header"], target, two_pass=True, append=False, records=False)
    with pytest.raises(ValueError):
        gpu_ctx.encode_frames([d], [k["header"]], [target], two_pass=[True, False])
    assert d.frame_count() == 0
    fi, _, _, updates = d.encode_frame(k["header"], target, two_pass=True)
    for bad in (updates[:2111], np.zeros(2113, np.uint8), np.zeros(1056, np.uint8)):
        with pytest.raises(ValueError):
            d.serialize_frame(fi, k["header"], k["ext"], optimise=True, first_pass_updates=bad)
    with pytest.raises(ValueError):
        gpu_ctx.serialize_frames([d], [fi], [k["header"]], [k["ext"]], optimise=True, first_pass_updates=[updates, updates])
    assert d.serialize_frame(fi, k["header"], k["ext"], optimise=True, first_pass_updates=updates) == k["bytes"]
    # append=False: the second pass's records come back, nothing is appended
    e = aa.Decoder(gpu_ctx, c["w"], c["h"])
    fi2, mb, blocks, u2 = e.encode_frame(k["header"], target, two_pass=True, append=False)
    assert fi2 == -1 and e.frame_count() == 0 and (u2 == updates).all()
    check_records("16x16_q93, append=False", k, mb, blocks)
