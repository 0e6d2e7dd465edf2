"""The forward encoder on the GPU (aa_encode_batch / Context.encode_frames; needs a real MI355X) against the reference's
xc-enc -i y4m -y QI -q best|rt, bit for bit, on the streams of tests/golden/reencode: pred.ivf frames 0..1 and c0.ivf frames 0..2 of every
case (tests/encode_model.py; the same comparison on the host: tests/test_encode_sim.py).

The header of each new frame is the product's parse of the fixture frame (quantiser, loop-filter level, refresh flags); every
macroblock's modes, reference, vectors / b_modes, flags, nz_mask, coeff_index, lf_level and all 25 x 16 coefficients must equal the parse
of the fixture frame.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import alfalfa_amd as aa
import encode_model as em
import make_y4m
import reencode_model as rmm
from alfalfa_amd import capi
from test_gpu_rebase import compare_records, device_target

pytestmark = pytest.mark.gpu


def decoder_before(ctx, name, which, k):
    """A decoder that has decoded the fixture's own frames 0 .. k-1 of the stream"""
    case = rmm.load_case(name)
    d = aa.Decoder(ctx, case["w"], case["h"])
    for data in case[which][:k]:
        d.parse_and_decode_frame(data)
    return d


def check_records(label, fr, got_mb, got_blocks):
    msg = compare_records(label, got_mb, got_blocks, fr["mb"], fr["dense"])
    assert msg is None, msg
    # what compare_records leaves out: the sub-block modes of EVERY intra macroblock, the loop-filter level, the segment, coeff_index
    want = fr["mb"]
    for f in ("u", "lf_level", "segment_id", "coeff_index", "flags"):
        bad = np.argwhere(np.array([[(got_mb[r, c][f] != want[r, c][f]).any() for c in range(want.shape[1])] for r in range(want.shape[0])]))
        assert len(bad) == 0, "%s: %s differs from the reference's at macroblocks (row, column) %s" % (label, f, bad[:6].tolist())
    assert len(got_blocks) == len(fr["blocks"]) and (got_blocks == fr["blocks"]).all(), "%s: the stored blocks differ" % label


def encode(ctx, which_frames, **kw):
    """The fixture frames `which_frames` [(name, which, k)] in ONE call, each on a decoder that decoded the fixture's frames before it
    -> [(decoder, result of encode_frames)]"""
    frs = [em.frames(n, w)[k] for n, w, k in which_frames]
    decs = [decoder_before(ctx, n, w, k) for n, w, k in which_frames]
    targets = [device_target(ctx, fr["target"]) for fr in frs]
    results = ctx.encode_frames(decs, [fr["header"] for fr in frs], targets, quality=[fr["quality_name"] for fr in frs], **kw)
    return list(zip(decs, results))


_single = {}


def single(ctx, name, which, k):
    """One fixture frame alone, checked against the reference and decoded -> (mb, blocks, raster); once per context."""
    key = (id(ctx), name, which, k)
    if key not in _single:
        fr = em.frames(name, which)[k]
        (d, (fi, mb, blocks)), = encode(ctx, [(name, which, k)])
        label = "%s %s.ivf frame %d (%s)" % (name, which, k, "key" if fr["key"] else "inter")
        check_records(label, fr, mb, blocks)
        assert fi == k and d.frame_count() == k + 1
        assert d.frame_header(fi)["key_frame"] == int(fr["key"])
        d.decode_frame(fi)
        raster = d.raster_bytes(fi)
        assert raster == b"".join(p.tobytes() for p in fr["decoded"]), "%s: records equal the reference's, the decoded planes are not what the fixture's bytes decode to" % label
        _single[key] = (mb, blocks, raster)
    return _single[key]


# ---- 1. every fixture frame, behind the fixture's own preceding frames ----
@pytest.mark.parametrize("which", ["pred", "c0"])
@pytest.mark.parametrize("name", em.CASES)
def test_encode_equals_the_reference(gpu_ctx, name, which):
    for k in range(em.STREAMS[which]):
        single(gpu_ctx, name, which, k)


# ---- 2. the whole stream from the decoder's own output ----
@pytest.mark.parametrize("which", ["pred", "c0"])
@pytest.mark.parametrize("name", em.CASES)
def test_the_stream_chained_from_its_own_key_frame(gpu_ctx, name, which):
    """Key, inter, inter -- every reference the decoder's own decode of the frame it encoded itself; the fixture's bytes are never parsed."""
    case = rmm.load_case(name)
    d = aa.Decoder(gpu_ctx, case["w"], case["h"])
    for k, fr in enumerate(em.frames(name, which)):
        fi, mb, blocks = d.encode_frame(fr["header"], device_target(gpu_ctx, fr["target"]), quality=fr["quality_name"])
        check_records("%s %s.ivf frame %d, chained" % (name, which, k), fr, mb, blocks)
        d.decode_frame(fi)
        assert d.raster_bytes(fi) == b"".join(p.tobytes() for p in fr["decoded"]), "%s %s.ivf frame %d, chained: decodes differently" % (name, which, k)


# ---- 3. all 35 frames in one call; capped rounds ----
def test_one_call_for_all_fixture_frames_and_capped_rounds_equal_the_single_runs(gpu_ctx):
    """Kinds, sizes and qualities mixed in one call; then with a round capped at one and at two macroblocks, so that the anti-diagonals
    of the 5 x 5 frames (up to three macroblocks) take several rounds."""
    want = [single(gpu_ctx, *f) for f in em.ALL]
    assert len(em.ALL) == 35
    try:
        for slots in (16, 1, 2):
            gpu_ctx.set_reencode_slots(slots)
            for f, (d, (fi, mb, blocks)), (wmb, wblocks, wraster) in zip(em.ALL, encode(gpu_ctx, em.ALL), want):
                assert (mb == wmb).all() and (blocks == wblocks).all(), "%d macroblocks per round, all frames in one call: %s differs from its single run" % (slots, f)
                d.decode_frame(fi)
                assert d.raster_bytes(fi) == wraster, "%d macroblocks per round: %s decodes differently" % (slots, f)
    finally:
        gpu_ctx.set_reencode_slots(16)


# ---- 4. diagonals longer than the slots: the hand-off between rounds ----
def test_560x288_at_16_slots_at_1_slot_and_on_the_host(gpu_ctx):
    """35 x 18 macroblocks: anti-diagonals of up to 18 macroblocks, more than the 16 slots of a round.  Key then inter, on twin decoders
    at 16 slots and at 1 slot, and by the host simulation from the decoder's own reference: the three record sets are byte-equal."""
    from test_encode_sim import sim_frame, sim_lib
    w, h, q = 560, 288, 40
    pictures = [em.pad(f, w, h) for f in make_y4m.synth_frames(w, h, 2, 5, "high")]
    template = em.frames("best_80x80", "pred")[0]["header"]
    got = {}
    try:
        for slots in (16, 1):
            gpu_ctx.set_reencode_slots(slots)
            d = aa.Decoder(gpu_ctx, w, h)
            out = []
            for k, planes in enumerate(pictures):
                hdr = em.header_like(template, w, h, q, key=k == 0)
                ref = [p.copy() for p in d.raster(k - 1)] if k else None
                fi, mb, blocks = d.encode_frame(hdr, device_target(gpu_ctx, planes), quality="best")
                d.decode_frame(fi)
                out.append((hdr, ref, mb, blocks, d.raster_bytes(fi)))
            got[slots] = out
    finally:
        gpu_ctx.set_reencode_slots(16)
    L = sim_lib()
    for k, planes in enumerate(pictures):
        hdr, ref, mb, blocks, raster = got[16][k]
        assert mb.shape == (18, 35)
        _, _, mb1, blocks1, raster1 = got[1][k]
        assert mb.tobytes() == mb1.tobytes() and blocks.tobytes() == blocks1.tobytes() and raster == raster1, "frame %d: 16 slots and 1 slot differ" % k
        fr = {"header": hdr, "target": planes, "ref": ref, "mv_probs": em.frames("best_80x80", "pred")[1]["mv_probs"], "quality": 0, "key": k == 0}
        smb, sdense, _ = sim_frame(L, fr)
        smb, sblocks = em.finished_records(smb, sdense, hdr["loop_filter_level"])
        assert mb.tobytes() == smb.tobytes() and blocks.tobytes() == sblocks.tobytes(), "frame %d: the kernel and the host simulation differ" % k


# ---- 6. bytes ----
def cleared(ext):
    """The fixture's header extension without what the probability passes decide (the library must recompute it)."""
    return dict(ext, token_prob_update=[0] * 1056, token_prob=[0] * 1056, skip_enabled=0, prob_skip_false=0, prob_inter=0, prob_references_last=0, prob_references_golden=0)


@pytest.mark.parametrize("which", ["pred", "c0"])
@pytest.mark.parametrize("name", ["best_72x40", "rt_80x80"])
def test_serialised_frames_are_the_fixture_s_bytes(gpu_ctx, name, which):
    """Frames 0 and 1: encode, serialize_frames( optimise=True, advance_state=True ) with the fixture's header extension, decode -- the
    bytes are the fixture's.  (Frame 2 of c0.ivf is pinned by its records: the reference reuses one InterFrame object, and header fields
    of the frame before can linger in its bytes.)"""
    case = rmm.load_case(name)
    d = aa.Decoder(gpu_ctx, case["w"], case["h"])
    for k, fr in enumerate(em.frames(name, which)[:2]):
        fi, mb, blocks = d.encode_frame(fr["header"], device_target(gpu_ctx, fr["target"]), quality=fr["quality_name"])
        data = d.serialize_frame(fi, fr["header"], fr["ext"], advance_state=True, optimise=True)
        want = fr["bytes"]
        assert data == want, "%s %s.ivf frame %d: %d bytes, the reference wrote %d; first difference at byte %d" % (
            name, which, k, len(data), len(want), next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), min(len(data), len(want))))
        d.decode_frame(fi)


def test_end_to_end_encode_search_serialise_parse_back(gpu_ctx):
    """encode -> lf_search_decode held to the fixture's level -> serialise -> the product's parser reads the same records back.  The
    search is the inter frames': aa_lf_search_decode_batch refuses a key frame (tests/test_gpu_lf_search_batch.py pins that), so the key
    frame carries the fixture's level in its header and is decoded plainly."""
    name, which = "best_72x40", "c0"
    case = rmm.load_case(name)
    d = aa.Decoder(gpu_ctx, case["w"], case["h"])
    p = aa.Parser(case["w"], case["h"])
    for k, fr in enumerate(em.frames(name, which)):
        level = fr["header"]["loop_filter_level"]
        target = device_target(gpu_ctx, fr["target"])
        if fr["key"]:
            fi, mb, blocks = d.encode_frame(fr["header"], target, quality=fr["quality_name"])
            d.decode_frame(fi)
        else:
            fi, mb, blocks = d.encode_frame(dict(fr["header"], loop_filter_level=(level + 5) % 64), target, quality=fr["quality_name"])      # (a provisional level)
            best, _, _ = d.lf_search_decode(fi, target, level_lo=level, level_hi=level)
            assert best == level
        hdr = d.frame_header(fi)
        assert hdr["loop_filter_level"] == level
        data = d.serialize_frame(fi, hdr, fr["ext"], advance_state=True, optimise=True)
        phdr, pmb, pblocks = p.parse(data)
        _, rmb, rblocks = d.read_records(fi)
        check_records("%s %s.ivf frame %d, end to end, parsed back" % (name, which, k), fr, pmb, pblocks)
        check_records("%s %s.ivf frame %d, end to end, as held" % (name, which, k), fr, rmb, rblocks)
        assert d.raster_bytes(fi) == b"".join(x.tobytes() for x in fr["decoded"])


# ---- 8. append=False ----
def test_without_append_nothing_is_appended_and_the_records_are_the_same(gpu_ctx):
    for f in (("best_72x40", "c0", 0), ("rt_80x80", "pred", 1)):
        wmb, wblocks, wraster = single(gpu_ctx, *f)
        (d, (fi, mb, blocks)), = encode(gpu_ctx, [f], append=False)
        assert fi == -1 and d.frame_count() == f[2], "append=False appended a frame"
        assert (mb == wmb).all() and (blocks == wblocks).all(), f
        # ... and they decode the same on a second decoder, once the caller appends them
        second = decoder_before(gpu_ctx, *f)
        fi2 = second.append_records(dict(em.frames(f[0], f[1])[f[2]]["header"]), mb, blocks)
        second.decode_frame(fi2)
        assert second.raster_bytes(fi2) == wraster, "%s: append_records of the returned records decodes differently" % (f,)


# ---- 7. refusals ----
def test_refusals_leave_every_stream_as_it_was(gpu_ctx):
    name = "best_16x16"
    case = rmm.load_case(name)
    key_fr, inter_fr = em.frames(name, "pred")[:2]
    key_hdr, inter_hdr = dict(key_fr["header"]), dict(inter_fr["header"])
    target = device_target(gpu_ctx, key_fr["target"])
    good, other = decoder_before(gpu_ctx, name, "pred", 1), decoder_before(gpu_ctx, name, "pred", 1)

    def refused(kind, text, decs, hdrs, targets):
        before = [d.frame_count() for d in decs]
        with pytest.raises(aa.AlfalfaError) as e:
            gpu_ctx.encode_frames(decs, hdrs, targets)
        assert e.value.kind == kind and e.value.message.startswith("aa_encode_batch: job 1:") and text in e.value.message, e.value
        assert [d.frame_count() for d in decs] == before, "a refused call appended a frame"

    # (the good job comes first in every call: it must not be appended either)
    refused("Unsupported", "segmentation", [good, other], [inter_hdr, dict(key_hdr, segmentation_enabled=1)], [target, target])
    refused("Unsupported", "segmentation", [good, other], [key_hdr, dict(inter_hdr, segmentation_enabled=1)], [target, target])
    big = rmm.load_case("best_72x40")
    refused("BadArgument", "dimensions", [good, aa.Decoder(gpu_ctx, big["w"], big["h"])], [inter_hdr, key_hdr], [target, device_target(gpu_ctx, big["targets"][0])])
    refused("BadArgument", "also job 0", [good, good], [inter_hdr, key_hdr], [target, target])
    fresh = aa.Decoder(gpu_ctx, case["w"], case["h"])
    refused("LogicError", "no decoded last reference", [good, fresh], [inter_hdr, inter_hdr], [target, target])
    pending = aa.Decoder(gpu_ctx, case["w"], case["h"])
    assert pending.encode_frame(key_hdr, target)[0] == 0                    # (a key job needs nothing before it)
    refused("LogicError", "not decoded", [good, pending], [inter_hdr, inter_hdr], [target, target])
    assert pending.encode_frame(key_hdr, target)[0] == 1                    # ... and is taken even behind a frame that is not decoded

    # the C call itself: null pointers, n = 0, a quality that is none, a coefficient array that is too small
    L = capi.lib()
    h = gpu_ctx._header_struct(inter_hdr)
    nmb = inter_hdr["mb_width"] * inter_hdr["mb_height"]
    out_mb = np.zeros(nmb, capi.MB_INFO_DTYPE)
    out_cf = np.zeros((25 * nmb, 16), np.int16)

    def job(dec, **kw):
        j = capi.EncodeJob()
        j.stream, j.hdr = dec.h, C.pointer(h)
        j.target.y, j.target.u, j.target.v = (t.data_ptr() for t in target)
        j.target.y_stride, j.target.uv_stride = case["pw"], case["pw"] // 2
        j.quality, j.append = 0, 1
        j.mbs_out, j.coeffs_out, j.coeff_capacity_blocks = out_mb.ctypes.data_as(C.c_void_p), out_cf.ctypes.data_as(C.c_void_p), len(out_cf)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    for broken in (job(other, mbs_out=None), job(other, hdr=None), job(other, stream=None), job(other, coeffs_out=None)):
        jobs = (capi.EncodeJob * 2)(job(good), broken)
        assert L.aa_encode_batch(gpu_ctx.h, jobs, 2) == -7 and b"aa_encode_batch: job 1: null pointer" in L.aa_last_error(), L.aa_last_error()
    jobs = (capi.EncodeJob * 2)(job(good), job(other, quality=2))
    assert L.aa_encode_batch(gpu_ctx.h, jobs, 2) == -7 and b"quality" in L.aa_last_error(), L.aa_last_error()
    assert L.aa_encode_batch(gpu_ctx.h, None, 1) == -7 and L.aa_encode_batch(gpu_ctx.h, jobs, 0) == -7
    jobs = (capi.EncodeJob * 2)(job(good), job(other, coeff_capacity_blocks=0))
    assert L.aa_encode_batch(gpu_ctx.h, jobs, 2) == -7 and b"too small" in L.aa_last_error(), L.aa_last_error()
    assert good.frame_count() == 1 and other.frame_count() == 1
    # ... and the same two decoders are still good for a call that is
    jobs = (capi.EncodeJob * 2)(job(good), job(other))
    assert L.aa_encode_batch(gpu_ctx.h, jobs, 2) == 0, L.aa_last_error()
    assert (jobs[0].frame_index, jobs[1].frame_index) == (1, 1) and jobs[0].num_coeff_blocks == jobs[1].num_coeff_blocks
    timing = gpu_ctx.encode_timing()
    assert timing["call_ms"] > 0 and timing["kernels_ms"] > 0
