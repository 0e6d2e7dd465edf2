"""The rebase on the GPU (aa_rebase_batch / Context.rebase; needs a real MI355X) against the reference's xc-enc -r, bit for bit, on the
fixtures of tests/golden/rebase (tests/golden/make_rebase_golden.py; their census: tests/test_rebase_model.py).

Per case: c0.state into a decoder, pred.ivf through a Parser, each new frame's header (quantiser factors, loop filter, refresh flags)
from the product's parse of rebased.ivf after c0.state, the edge-extended target uploaded; then frame by frame rebase and decode.
Every frame, every macroblock: the 25 x 16 coefficients equal the parse of rebased.ivf, modes / references / vectors / b_modes /
partition and the five flags are equal, and the decoded padded planes hash to rebase_golden.json.  A difference is reported by frame,
macroblock, class and block index."""
import collections
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import alfalfa_amd as aa
import rebase_model as rm
from alfalfa_amd import capi

pytestmark = pytest.mark.gpu
FLAGS = (("HAS_NONZERO", 1), ("HAS_Y2", 2), ("INTER", 4), ("SKIP", 8), ("LF_SKIP_INNER", 16))

_loaded = {}


def fixture_of(name):
    """-> (case, [(header, mb, blocks)] of pred.ivf, the same of rebased.ivf, [dense coefficients of the rebased frames]): made once."""
    if name not in _loaded:
        case = rm.load_case(name)
        pred, rebased = rm.parse_frames(case, "pred"), rm.parse_frames(case, "rebased")
        _loaded[name] = (case, pred, rebased, [rm.dense(mb, blocks) for _, mb, blocks in rebased])
    return _loaded[name]


def fresh_decoder(ctx, case):
    d = aa.Decoder(ctx, case["w"], case["h"])
    d.deserialize(case["state"])
    return d


def device_target(ctx, planes):
    dev = torch.device("cuda", ctx.device)
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in planes)


def compare_records(label, got_mb, got_blocks, want_mb, want_dense):
    """The message for a frame whose records differ from the reference's, or None."""
    got_dense = rm.dense(got_mb, got_blocks)
    bad, classes = [], collections.Counter()
    for r in range(want_mb.shape[0]):
        for c in range(want_mb.shape[1]):
            g, w = got_mb[r, c], want_mb[r, c]
            what = [f for f in ("y_mode", "uv_mode", "ref_frame", "split_partition") if g[f] != w[f]]
            if w["ref_frame"] != 0 and (g["u"] != w["u"]).any():
                what.append("vectors")
            if w["y_mode"] == rm.B_PRED and (g["u"][:16] != w["u"][:16]).any():
                what.append("b_modes")
            what += ["flag " + n for n, bit in FLAGS if (g["flags"] ^ w["flags"]) & bit]
            if g["nz_mask"] != w["nz_mask"]:
                what.append("nz_mask %07x want %07x" % (g["nz_mask"], w["nz_mask"]))
            for b in range(25):
                if (got_dense[r, c, b] != want_dense[r, c, b]).any():
                    what.append("block %d: %s want %s" % (b, got_dense[r, c, b].tolist(), want_dense[r, c, b].tolist()))
                    break
            if what:
                bad.append("  macroblock (%d, %d) %s: %s" % (c, r, rm.describe(w), "; ".join(what)))
                classes[rm.describe(w).split(" mv")[0]] += 1
    if not bad:
        return None
    return "\n".join(["%s: %d macroblocks differ from the reference (%s)" % (label, len(bad), ", ".join("%d %s" % (n, k) for k, n in classes.most_common()))] + bad[:6])


def run_case(ctx, name, decoders=None):
    """Rebase and decode every frame of a case on one decoder (or on each of `decoders`, in one call per frame) and check everything."""
    case, pred, rebased, want_dense = fixture_of(name)
    decs = decoders or [fresh_decoder(ctx, case)]
    out = []
    for k, (hdr, want_mb, _) in enumerate(rebased):
        target = device_target(ctx, case["targets"][k])
        results = ctx.rebase(decs, [hdr] * len(decs), [pred[k + 1][1]] * len(decs), [target] * len(decs))
        ctx.decode_batch(decs, [fi for fi, _, _ in results])
        for d, (fi, mb, blocks) in zip(decs, results):
            msg = compare_records("%s frame %d" % (name, k), mb, blocks, want_mb, want_dense[k])
            assert msg is None, msg
            raster = d.raster_bytes(fi)
            assert hashlib.sha256(raster).hexdigest() == case["sha256"][k], "%s frame %d: records equal the reference's, the decoded planes do not hash to the golden" % (name, k)
            out.append((mb, blocks, raster))
    return out


@pytest.mark.parametrize("name", rm.CASES)
def test_rebase_equals_the_reference(gpu_ctx, name):
    run_case(gpu_ctx, name)


BATCH = ["dir_split_80x48", "dir_fraction_80x48", "dir_edge_80x48", "dir_wave_80x48", "enc_skip_80x48"]


def lock_step(ctx, names):
    """All `names` (one size) through Context.rebase in lock step, one job per case and call; cases that run out of frames drop out."""
    fx = [fixture_of(n) for n in names]
    decs = [fresh_decoder(ctx, f[0]) for f in fx]
    got = [[] for _ in names]
    for k in range(max(len(f[2]) for f in fx)):
        live = [i for i, f in enumerate(fx) if k < len(f[2])]
        targets = [device_target(ctx, fx[i][0]["targets"][k]) for i in live]
        results = ctx.rebase([decs[i] for i in live], [fx[i][2][k][0] for i in live], [fx[i][1][k + 1][1] for i in live], targets)
        ctx.decode_batch([decs[i] for i in live], [r[0] for r in results])
        for i, (fi, mb, blocks) in zip(live, results):
            got[i].append((mb, blocks, decs[i].raster_bytes(fi)))
    return got


def same(a, b):
    return len(a) == len(b) and all((x[0] == y[0]).all() and (x[1] == y[1]).all() and x[2] == y[2] for x, y in zip(a, b))


def test_batches_equal_the_single_decoder_runs(gpu_ctx, monkeypatch):
    single = {n: run_case(gpu_ctx, n) for n in BATCH}
    for i, got in enumerate(lock_step(gpu_ctx, BATCH)):                       # five jobs per call
        assert same(got, single[BATCH[i]]), "batch of five: %s differs from its single-decoder run" % BATCH[i]
    # two copies of each: ten jobs, and a dense scratch bounded to 40 000 bytes -- 12 000 per job here -- so that the call works through
    # them in slices of three jobs and a last one of one
    monkeypatch.setenv("ALFALFA_AMD_REBASE_SLICE_BYTES", "40000")
    for i, got in enumerate(lock_step(gpu_ctx, BATCH + BATCH)):
        assert same(got, single[(BATCH + BATCH)[i]]), "batch of ten in slices: copy %d of %s differs from its single-decoder run" % (i // 5, (BATCH + BATCH)[i])


def test_returned_records_decode_the_same_on_a_second_decoder(gpu_ctx):
    for name in ("dir_split_80x48", "enc_best_72x40"):
        case, pred, rebased, _ = fixture_of(name)
        first = run_case(gpu_ctx, name)
        second = fresh_decoder(gpu_ctx, case)
        for k, (mb, blocks, raster) in enumerate(first):
            fi = second.append_records(dict(rebased[k][0]), mb, blocks)
            second.decode_frame(fi)
            assert second.raster_bytes(fi) == raster, "%s frame %d: append_records of the returned records decodes differently" % (name, k)


def test_refusals_leave_every_stream_as_it_was(gpu_ctx):
    case, pred, rebased, _ = fixture_of("dir_split_16x16")
    hdr, mb = dict(rebased[0][0]), pred[1][1]
    target = device_target(gpu_ctx, case["targets"][0])
    good, other = fresh_decoder(gpu_ctx, case), fresh_decoder(gpu_ctx, case)

    def refused(kind, text, decs, hdrs, mbs, targets):
        before = [d.frame_count() for d in decs]
        with pytest.raises(aa.AlfalfaError) as e:
            gpu_ctx.rebase(decs, hdrs, mbs, targets)
        assert e.value.kind == kind and "aa_rebase_batch" in e.value.message and text in e.value.message, e.value
        assert [d.frame_count() for d in decs] == before, "a refused call appended a frame"

    # (the good job comes first in every call: it must not be appended either)
    refused("BadArgument", "key frame", [good, other], [hdr, dict(hdr, key_frame=1)], [mb, mb], [target, target])
    refused("Unsupported", "segmentation", [good, other], [hdr, dict(hdr, segmentation_enabled=1)], [mb, mb], [target, target])
    refused("BadArgument", "dimensions", [good, other], [hdr, dict(hdr, mb_width=hdr["mb_width"] + 1)], [mb, np.concatenate([mb, mb], 1)], [target, target])
    refused("BadArgument", "also job 0", [good, good], [hdr, hdr], [mb, mb], [target, target])
    pending = fresh_decoder(gpu_ctx, case)
    pending.append_records(dict(rebased[0][0]), rebased[0][1], rebased[0][2])
    refused("LogicError", "not decoded", [good, pending], [hdr, hdr], [mb, mb], [target, target])

    # the C call itself: null pointers, and a coefficient array that is too small (the message names the count needed)
    L = capi.lib()
    h = capi.FrameHeader()
    for n, _ in capi.FrameHeader._fields_:
        if n != "quant":
            setattr(h, n, hdr[n])
    for s in range(4):
        for k in range(6):
            h.quant[s][k] = hdr["quant"][s][k]
    rec = np.ascontiguousarray(mb).reshape(-1)
    out_mb = np.zeros(len(rec), capi.MB_INFO_DTYPE)
    out_cf = np.zeros((25 * len(rec), 16), np.int16)

    def job(dec, **kw):
        j = capi.RebaseJob()
        j.stream, j.hdr, j.mbs = dec.h, C.pointer(h), rec.ctypes.data_as(C.c_void_p)
        j.target.y, j.target.u, j.target.v = (t.data_ptr() for t in target)
        j.target.y_stride, j.target.uv_stride = case["pw"], case["pw"] // 2
        j.mbs_out, j.coeffs_out, j.coeff_capacity_blocks = out_mb.ctypes.data_as(C.c_void_p), out_cf.ctypes.data_as(C.c_void_p), len(out_cf)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    for broken in (job(other, mbs=None), job(other, mbs_out=None), job(other, hdr=None), job(other, stream=None)):
        jobs = (capi.RebaseJob * 2)(job(good), broken)
        assert L.aa_rebase_batch(gpu_ctx.h, jobs, 2) == -7 and b"null pointer" in L.aa_last_error(), L.aa_last_error()
    assert L.aa_rebase_batch(gpu_ctx.h, None, 1) == -7
    need = gpu_ctx.rebase([fresh_decoder(gpu_ctx, case)], [hdr], [mb], [target])[0][2].shape[0]
    assert need > 1
    jobs = (capi.RebaseJob * 2)(job(good), job(other, coeff_capacity_blocks=need - 1))
    assert L.aa_rebase_batch(gpu_ctx.h, jobs, 2) == -7
    assert b"too small" in L.aa_last_error() and (b"%d blocks needed" % need) in L.aa_last_error(), L.aa_last_error()
    assert good.frame_count() == 0 and other.frame_count() == 0
    # ... and the same two decoders are still good for a call that is
    out_mb2, out_cf2 = np.zeros_like(out_mb), np.zeros_like(out_cf)
    jobs = (capi.RebaseJob * 2)(job(good), job(other, mbs_out=out_mb2.ctypes.data_as(C.c_void_p), coeffs_out=out_cf2.ctypes.data_as(C.c_void_p)))
    assert L.aa_rebase_batch(gpu_ctx.h, jobs, 2) == 0, L.aa_last_error()
    assert (jobs[0].frame_index, jobs[1].frame_index, jobs[1].num_coeff_blocks) == (0, 0, need)
    assert (out_mb == out_mb2).all() and (out_cf == out_cf2).all()
