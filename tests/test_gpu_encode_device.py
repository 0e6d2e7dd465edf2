"""The forward encoder with the new frame's records compacted and kept on the GPU (aa_encode_device_batch / Context.encode_frames(
records=False ); needs a real MI355X): k_reencode_count and k_reencode_compact behind k_encode_key / k_encode_inter, the frame in a piece
of HBM of its own.  The reference is aa_encode_batch, itself pinned to the reference's encoder by tests/test_gpu_encode.py: on twin
decoders Decoder.read_records gives the same bytes, key frames and inter frames alike, and the frames decode, rewind and release like
re-encoded ones."""
import ctypes as C

import numpy as np
import pytest

import alfalfa_amd as aa
import encode_model as em
import reencode_model as rmm
from alfalfa_amd import capi
from test_gpu_encode import check_records, decoder_before
from test_gpu_rebase import device_target

pytestmark = pytest.mark.gpu


def twins(ctx, which_frames, slots=16):
    """The fixture frames [(name, which, k)] in one call of each kind on twin decoders -> [(device decoder, fi, host decoder, fi, returned mb, returned blocks)]"""
    frs = [em.frames(n, w)[k] for n, w, k in which_frames]
    new, old = [decoder_before(ctx, *f) for f in which_frames], [decoder_before(ctx, *f) for f in which_frames]
    targets = [device_target(ctx, fr["target"]) for fr in frs]
    headers, quality = [fr["header"] for fr in frs], [fr["quality_name"] for fr in frs]
    try:
        ctx.set_reencode_slots(slots)
        dev = ctx.encode_frames(new, headers, targets, quality=quality, records=False)
        host = ctx.encode_frames(old, headers, targets, quality=quality)
    finally:
        ctx.set_reencode_slots(16)
    return [(n, fi, o, fo, mb, blocks, count) for n, (fi, count), o, (fo, mb, blocks) in zip(new, dev, old, host)]


@pytest.mark.parametrize("slots", [16, 2])
def test_twin_decoders_hold_the_same_bytes_for_all_fixture_frames_in_one_call(gpu_ctx, slots):
    """All 35 frames, kinds mixed: byte for byte what Decoder.read_records gives after the host-record call, and what that call returned."""
    out = twins(gpu_ctx, em.ALL, slots)
    gpu_ctx.decode_batch([t[0] for t in out] + [t[2] for t in out], [t[1] for t in out] + [t[3] for t in out])
    for f, (new, fi, old, fo, mb, blocks, count) in zip(em.ALL, out):
        fr = em.frames(f[0], f[1])[f[2]]
        assert fi == fo == f[2]
        hn, mbn, bn = new.read_records(fi)
        ho, mbo, bo = old.read_records(fo)
        assert mbn.tobytes() == mbo.tobytes() == np.ascontiguousarray(mb).tobytes(), "%s: the 80-byte records differ" % (f,)
        assert bn.tobytes() == bo.tobytes() == blocks.tobytes() and count == len(bn), "%s: the coefficient blocks differ" % (f,)
        for field in ("key_frame", "num_coeff_blocks", "num_intra_mbs", "has_intra_mb", "num_macroblocks", "loop_filter_level", "q_index"):
            assert hn[field] == ho[field], (f, field)
        assert hn["key_frame"] == int(fr["key"]) and hn["num_intra_mbs"] == int((mbn["ref_frame"] == 0).sum())
        check_records("%s, device-resident" % (f,), fr, mbn, bn)
        assert new.raster_bytes(fi) == old.raster_bytes(fo) == b"".join(p.tobytes() for p in fr["decoded"]), "%s: the decoded planes differ" % (f,)


def test_without_records_a_frame_is_always_appended(gpu_ctx):
    f = ("best_16x16", "pred", 0)
    fr = em.frames(*f[:2])[0]
    d = decoder_before(gpu_ctx, *f)
    target = device_target(gpu_ctx, fr["target"])
    with pytest.raises(ValueError):
        gpu_ctx.encode_frames([d], [fr["header"]], [target], records=False, append=False)
    with pytest.raises(ValueError):
        d.encode_frame(fr["header"], target, records=False, append=False)
    assert d.frame_count() == 0


def test_rewind_release_and_the_stream_goes_on(gpu_ctx):
    """Key and two inter frames kept on the device; the stream rewinds to its key frame and decodes the same, a released frame's records
    are gone, and the stream goes on."""
    name, which = "best_72x40", "c0"
    case = rmm.load_case(name)
    frs = em.frames(name, which)
    d = aa.Decoder(gpu_ctx, case["w"], case["h"])
    fis = []
    for fr in frs:
        fi, count = d.encode_frame(fr["header"], device_target(gpu_ctx, fr["target"]), quality=fr["quality_name"], records=False)
        assert count == len(fr["blocks"])
        d.decode_frame(fi)
        fis.append(fi)
    assert fis == [0, 1, 2]
    rasters = [d.raster_bytes(fi) for fi in fis]
    assert rasters == [b"".join(p.tobytes() for p in fr["decoded"]) for fr in frs]
    d.rewind_to(0)
    for fi in fis:
        d.decode_frame(fi)
    assert [d.raster_bytes(fi) for fi in fis] == rasters, "after rewind_to the encoded key frame the stream decodes differently"
    d.release_staging()
    _, mb0, blocks0 = d.read_records(0)
    check_records("%s %s.ivf frame 0, read back after release_staging" % (name, which), frs[0], mb0, blocks0)
    d.release_frame(0)
    with pytest.raises(aa.AlfalfaError) as e:
        d.read_records(0)
    assert "released" in e.value.message
    d.release_before(3)
    with pytest.raises(aa.AlfalfaError) as e:
        d.read_records(2)
    assert "released" in e.value.message
    # ... and the stream goes on: the third picture again, predicted from the decode of itself
    fi, count = d.encode_frame(frs[2]["header"], device_target(gpu_ctx, frs[2]["target"]), quality=frs[2]["quality_name"], records=False)
    d.decode_frame(fi)
    assert fi == 3 and count == len(d.read_records(fi)[2]) and len(d.raster_bytes(fi))


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
            gpu_ctx.encode_frames(decs, hdrs, targets, records=False)
        assert e.value.kind == kind and e.value.message.startswith("aa_encode_device_batch: job 1:") and text in e.value.message, e.value
        assert [d.frame_count() for d in decs] == before, "a refused call appended a frame"

    refused("Unsupported", "segmentation", [good, other], [inter_hdr, dict(key_hdr, segmentation_enabled=1)], [target, target])
    refused("BadArgument", "also job 0", [good, good], [inter_hdr, key_hdr], [target, target])
    fresh = aa.Decoder(gpu_ctx, case["w"], case["h"])
    refused("LogicError", "no decoded last reference", [good, fresh], [inter_hdr, inter_hdr], [target, target])
    pending = aa.Decoder(gpu_ctx, case["w"], case["h"])
    assert pending.encode_frame(key_hdr, target, records=False)[0] == 0
    refused("LogicError", "not decoded", [good, pending], [inter_hdr, inter_hdr], [target, target])
    L = capi.lib()
    h = gpu_ctx._header_struct(inter_hdr)
    j = capi.EncodeDeviceJob()
    j.stream, j.hdr, j.quality = good.h, C.pointer(h), 0
    j.target.y, j.target.u, j.target.v = (t.data_ptr() for t in target)
    j.target.y_stride, j.target.uv_stride = case["pw"], case["pw"] // 2
    broken = capi.EncodeDeviceJob()
    C.memmove(C.byref(broken), C.byref(j), C.sizeof(j))
    broken.stream, broken.hdr = other.h, None
    jobs = (capi.EncodeDeviceJob * 2)(j, broken)
    assert L.aa_encode_device_batch(gpu_ctx.h, jobs, 2) == -7 and b"aa_encode_device_batch: job 1: null pointer" in L.aa_last_error(), L.aa_last_error()
    assert good.frame_count() == 1 and other.frame_count() == 1
    timing_before = gpu_ctx.encode_timing()
    assert good.encode_frame(inter_hdr, target, records=False)[0] == 1
    timing = gpu_ctx.encode_timing()
    assert timing["call_ms"] > 0 and timing["kernels_ms"] > 0 and timing["records_ms"] == 0 and timing != timing_before
