"""The serialisation on the GPU (aa_serialize_batch / Context.serialize_frames; needs a real MI355X): records -> VP8 frames, the DCT
partitions written by k_serialize_tokens, against frames the reference's Frame::serialize wrote -- byte for byte.

  * the chunks of tests/golden/rebase and tests/golden/reencode: from c0.state every frame is made by the rebase (frame 0 of a re-encode
    case by the re-encode), serialised with optimise set and the header the reference wrote for it (parsed from rebased.ivf) with every
    field the probability passes decide CLEARED -- token probability updates, prob_skip_false, and each of the three reference
    probabilities that optimize_interframe_probs sets for the frame (it leaves a field alone where calc_prob gives 0: what the reference
    wrote there is not recomputable and stays) -- against the stream's own state, which follows every written frame (advance_state), and
    decoded: every frame is rebased.ivf's frame, the header handed back is the reference's, and the counts k_token_counts made are the
    numpy model's (tests/serialize_model.py), table for table;
  * the fixed point: every stream of tests/golden/serialize_fixed_point.json (the streams the reference's own parse -> serialise
    reproduces, tests/test_bool_writer.py), parsed by the host AND by the device parser (packed or dense records, by the context), is
    written back as its own bytes;
  * the semantic round trip on the synthetic feature streams (segmentation with map updates, SPLITMV, golden / altref with sign bias,
    B_PRED, hidden frames, probability updates, several partitions): whatever the partition count asked for, the written frame parses
    to the same records, header, rest of the header and state, and decodes to the same raster;
  * refusals leave `out`, its guard bytes and every stream's state as they were."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import alfalfa_amd as aa
import rebase_model as rm
import reencode_model as rmm
import serialize_model as sm
from alfalfa_amd import capi
from conftest import GOLDEN_DIR, golden_frames
from test_gpu_rebase import device_target

pytestmark = pytest.mark.gpu

FIXED_POINT = json.load(open(os.path.join(GOLDEN_DIR, "serialize_fixed_point.json")))["reproduced_by_reference"]
SYNTH = ["synth_33x17_s7", "synth_64x64_s20", "synth_200x48_s11", "synth_96x80_s1", "synth_175x143_s3"]

_walk = {}


def walk(key, w, h, frames, state=None):
    """A host parser over `frames` (continuing from `state`, the reference's DecoderState bytes) -> per frame (header, rest of the header,
    sub-block modes, tables before, mb, blocks, parser state after); made once per key."""
    if key not in _walk:
        p = aa.Parser(w, h)
        if state is not None:
            p.deserialize_state(state)
        out = []
        for fr in frames:
            before = p.probs().copy()
            hdr, mb, blocks = p.parse(fr)
            out.append((hdr, p.header_ext(), p.sub_modes().copy(), before, mb, blocks, p.export_state()))
        _walk[key] = out
    return _walk[key]


def fresh_decoder(ctx, case):
    d = aa.Decoder(ctx, case["w"], case["h"])
    d.deserialize(case["state"])
    return d


def chunk_plan(kind, name):
    """-> (case, per frame (header, ext, sub-block modes of the prediction frame, prediction records or None = re-encode, parser state after))"""
    if kind == "rebase":
        case = rm.load_case(name)
        pred = walk(("pred", kind, name), case["w"], case["h"], case["pred"])[1:]
    else:
        case = rmm.load_case(name)
        pred = walk(("pred", kind, name), case["w"], case["h"], case["pred"])
    ref = walk(("rebased", kind, name), case["w"], case["h"], case["rebased"], rm.decoder_state(case))
    plan = []
    for k, (hdr, ext, _, _, mb, blocks, after) in enumerate(ref):
        reencode = kind == "reencode" and k == 0
        plan.append((hdr, cleared(ext, mb), None if reencode else pred[k][2], None if reencode else pred[k][4], after, ext, mb, blocks))
    return case, plan


def cleared(ext, mb):
    """The reference's header without what the probability passes decide for this frame (the library must recompute it)."""
    x = dict(ext, token_prob_update=[0] * 1056, token_prob=[0] * 1056, skip_enabled=0, prob_skip_false=0)
    for field, decided in zip(("prob_inter", "prob_references_last", "prob_references_golden"), sm.frame_probs(mb)[1:]):
        if decided:
            x[field] = 0
    return x


def model_counts(mb, blocks):
    """What aa_serialize_job::counts_out holds, from the model: branch counts, macroblocks with coefficients, macroblocks by reference."""
    out = np.zeros(2120, np.uint32)
    out[:2112] = sm.branch_counts(mb, blocks).reshape(-1)
    out[2112] = int(((mb["nz_mask"] != 0) & ((mb["flags"] & 8) == 0)).sum())
    out[2113:2117] = [int((mb["ref_frame"] == k).sum()) for k in range(4)]
    return out


def make_frame(ctx, d, case, step, k):
    hdr, ext, subs, pred_mb = step[:4]
    target = device_target(ctx, case["targets"][k])
    if pred_mb is None:
        return d.reencode_as_inter(hdr, target, quality=case["quality"])[0]
    return d.rebase(hdr, pred_mb, target)[0]


CHUNKS = [("rebase", n) for n in rm.CASES] + [("reencode", n) for n in rmm.CASES]


@pytest.mark.parametrize("kind,name", CHUNKS)
def test_a_chunk_is_the_reference_s_bytes(gpu_ctx, kind, name):
    case, plan = chunk_plan(kind, name)
    d = fresh_decoder(gpu_ctx, case)
    for k, step in enumerate(plan):
        fi = make_frame(gpu_ctx, d, case, step, k)
        data, written, counts = d.serialize_frame(fi, step[0], step[1], advance_state=True, sub_modes=step[2], optimise=True, details=True)
        want = case["rebased"][k]
        bad = np.flatnonzero(counts != model_counts(step[6], step[7]))
        assert len(bad) == 0, "%s %s frame %d: k_token_counts differs from the model at %s (node * 2 + taken; 2112.. the macroblock classes)" % (kind, name, k, bad[:8].tolist())
        assert written == step[5], "%s %s frame %d: the header handed back differs from the reference's in %s" % (kind, name, k, [f for f in written if written[f] != step[5][f]])
        assert data == want, "%s %s frame %d: %d bytes, the reference wrote %d; first difference at byte %d" % (
            kind, name, k, len(data), len(want), next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), min(len(data), len(want))))
        assert d.export_state() == step[4], "%s %s frame %d: the decoder's state did not follow the written frame as a parse of it does" % (kind, name, k)
        d.decode_frame(fi)
        assert hashlib.sha256(d.raster_bytes(fi)).hexdigest() == case["sha256"][k]


def test_all_chunks_in_one_call_per_step(gpu_ctx):
    """Every fixture in lock step: frame k of all chunks that have one is serialised by ONE call (mixed sizes, fifteen jobs at first)."""
    plans = [chunk_plan(kind, name) for kind, name in CHUNKS]
    decs = [fresh_decoder(gpu_ctx, case) for case, _ in plans]
    for k in range(max(len(p) for _, p in plans)):
        live = [i for i, (_, p) in enumerate(plans) if k < len(p)]
        fis = [make_frame(gpu_ctx, decs[i], plans[i][0], plans[i][1][k], k) for i in live]
        got = gpu_ctx.serialize_frames([decs[i] for i in live], fis, [plans[i][1][k][0] for i in live], [plans[i][1][k][1] for i in live], advance_state=True,
                                       sub_modes=[plans[i][1][k][2] for i in live], optimise=True)
        for i, data in zip(live, got):
            assert data == plans[i][0]["rebased"][k], "step %d, %d jobs in one call: %s %s differs from the reference's frame" % (k, len(live), CHUNKS[i][0], CHUNKS[i][1])
        gpu_ctx.decode_batch([decs[i] for i in live], fis)


@pytest.mark.parametrize("name", FIXED_POINT)
def test_parse_then_serialise_is_the_identity(gpu_ctx, name):
    """Host-parsed records (dense, in the stream's frame store) and device-parsed records (the context's format, in the coefficient heap) of
    the same frame in one call: both are written back as the frame's own bytes, key frames included."""
    w, h, frames = golden_frames(name)
    steps = walk(("golden", name), w, h, frames)
    host, dev = aa.Decoder(gpu_ctx, w, h), aa.Decoder(gpu_ctx, w, h)
    dev_fis = gpu_ctx.submit_frames([(dev, fr) for fr in frames], route="device")
    for k, (fr, (hdr, ext, subs, before, _, _, _)) in enumerate(zip(frames, steps)):
        fi, _ = host.parse_frame(fr)
        got = gpu_ctx.serialize_frames([host, dev], [fi, dev_fis[k]], [hdr, hdr], [ext, ext], probs_before=[before, before], sub_modes=[subs, subs])
        for how, data in zip(("host-parsed", "device-parsed"), got):
            assert data == fr, "%s frame %d (%s, %s): %d bytes written back as %d, first difference at byte %d" % (
                name, k, "key" if hdr["key_frame"] else "inter", how, len(fr), len(data), next((i for i, (a, b) in enumerate(zip(data, fr)) if a != b), min(len(data), len(fr))))


def same_header(a, b):
    skip = ("num_dct_partitions", "compressed_size")
    return all(a[f] == b[f] for f in a if f not in skip)


@pytest.mark.parametrize("name", SYNTH)
def test_any_partition_count_parses_back_to_the_same_frame(gpu_ctx, name):
    w, h, frames = golden_frames(name)
    steps = walk(("golden", name), w, h, frames)
    dev = aa.Decoder(gpu_ctx, w, h)
    fis = gpu_ctx.submit_frames([(dev, fr) for fr in frames], route="device")
    original = aa.Decoder(gpu_ctx, w, h)
    rasters = []
    for fr in frames:
        _, fi = original.get_frame_output(fr)
        rasters.append(original.raster_bytes(fi))
    for parts in (1, 2, 4, 8):
        back, again = aa.Parser(w, h), aa.Decoder(gpu_ctx, w, h)
        for k, (hdr, ext, subs, before, mb, blocks, after) in enumerate(steps):
            data = dev.serialize_frame(fis[k], dict(hdr, num_dct_partitions=parts), ext, probs_before=before)      # (no sub-block modes: the first that fits)
            hdr2, mb2, blocks2 = back.parse(data)
            what = "%s frame %d as %d partitions" % (name, k, parts)
            assert hdr2["num_dct_partitions"] == parts and same_header(hdr, hdr2), "%s: the header parses back as %s, was %s" % (what, hdr2, hdr)
            assert back.header_ext() == ext, "%s: the rest of the header parses back differently" % what
            assert (mb2 == mb).all() and (blocks2 == blocks).all(), "%s: the records parse back differently" % what
            assert back.export_state() == after, "%s: the state after the frame differs" % what
            _, fi = again.get_frame_output(data)
            assert again.raster_bytes(fi) == rasters[k], "%s: decodes to another raster" % what


def test_refusals_write_nothing_and_advance_nothing(gpu_ctx):
    kind, name = "rebase", "dir_split_16x16"
    case, plan = chunk_plan(kind, name)
    good, other = fresh_decoder(gpu_ctx, case), fresh_decoder(gpu_ctx, case)
    fis = [make_frame(gpu_ctx, d, case, plan[0], 0) for d in (good, other)]
    hdr, ext, subs = plan[0][0], plan[0][5], plan[0][2]          # (the reference's own header, written as given: optimise clear)
    want = case["rebased"][0]
    L = capi.lib()
    h = gpu_ctx._header_struct(hdr)
    x = capi.FrameHeaderExt.from_dict(ext)
    sm = np.ascontiguousarray(subs, dtype=np.uint8)
    bufs = [np.full(len(want) + 64, 0xA5, np.uint8) for _ in range(2)]
    probs = np.zeros(1101, np.uint8)

    def job(dec, fi, buf, **kw):
        j = capi.SerializeJob()
        j.stream, j.frame_index, j.hdr, j.ext = dec.h, fi, C.pointer(h), C.pointer(x)
        j.advance_state = 1
        j.sub_modes, j.num_sub_modes = (sm.ctypes.data_as(C.c_void_p), len(sm)) if len(sm) else (None, 0)
        j.out, j.capacity = buf.ctypes.data_as(C.c_void_p), len(want)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def state_hash(d):
        v = C.c_uint64()
        capi.check(L.aa_stream_state_hash(d.h, C.byref(v)))
        return v.value

    def refused(code, text, second):
        states = [d.export_state() for d in (good, other)]
        hashes = [state_hash(d) for d in (good, other)]
        jobs = (capi.SerializeJob * 2)(job(good, fis[0], bufs[0]), second)      # (the good job comes first: it must not be written either)
        assert L.aa_serialize_batch(gpu_ctx.h, jobs, 2) == code, L.aa_last_error()
        msg = L.aa_last_error()
        assert b"aa_serialize_batch" in msg and text in msg, msg
        assert all((b == 0xA5).all() for b in bufs), "a refused call wrote into an output buffer: " + msg.decode()
        assert [d.export_state() for d in (good, other)] == states and [state_hash(d) for d in (good, other)] == hashes, "a refused call advanced a state"

    h8 = gpu_ctx._header_struct(dict(hdr, num_dct_partitions=3))
    hw = gpu_ctx._header_struct(dict(hdr, mb_width=hdr["mb_width"] + 1))
    refused(-7, b"%d bytes needed, room for %d" % (len(want), len(want) - 1), job(other, fis[1], bufs[1], capacity=len(want) - 1))
    refused(-7, b"also job 0", job(good, fis[0], bufs[1]))
    refused(-7, b"advance_state together with probs_before", job(other, fis[1], bufs[1], probs_before=probs.ctypes.data_as(C.c_void_p)))
    refused(-7, b"1, 2, 4 or 8", job(other, fis[1], bufs[1], hdr=C.pointer(h8)))
    refused(-7, b"dimensions", job(other, fis[1], bufs[1], hdr=C.pointer(hw)))
    refused(-7, b"out of range", job(other, 7, bufs[1]))
    refused(-7, b"null pointer", job(other, fis[1], bufs[1], ext=None))
    refused(-7, b"null pointer", job(other, fis[1], bufs[1], out=None))
    assert L.aa_serialize_batch(gpu_ctx.h, None, 1) == -7
    # ... and the same two decoders are still good for a call that is: exactly the capacity needed, guard bytes untouched
    jobs = (capi.SerializeJob * 2)(job(good, fis[0], bufs[0]), job(other, fis[1], bufs[1]))
    assert L.aa_serialize_batch(gpu_ctx.h, jobs, 2) == 0, L.aa_last_error()
    for j, b in zip(jobs, bufs):
        assert j.size == len(want) and b[:len(want)].tobytes() == want and (b[len(want):] == 0xA5).all()
    assert good.export_state() == other.export_state() == plan[0][4]
    timing = gpu_ctx.serialize_timing()
    assert timing["call_ms"] > 0 and timing["kernel_ms"] > 0
