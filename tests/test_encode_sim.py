"""The forward encoder's decision on the host (tests/cpp/encode_sim.cc: reencode_search.hh under KeyPolicy and ForwardInterPolicy,
reencode_mb.hh and rebase_inl.hh, the statements the lanes of k_encode_key / k_encode_inter run, one lane at a time) against the reference's
xc-enc -i y4m -y QI -q best|rt on the streams of tests/golden/reencode: every mode, vector, b_mode and uv_mode and every coefficient of
pred.ivf frames 0..1 and c0.ivf frames 0..2 of every case -- key frames and forward inter frames, the inter frames predicted from the
oracle's decode of the fixture frames before them.  CPU only; the GPU run of the same comparison is tests/test_gpu_encode.py.  The same
program, stand-alone and under AddressSanitizer / UBSan, runs over the same inputs.  And the host's side of a job's cost block --
update_rd_multipliers, fill_mv_sad_costs -- against the reference's written formulas, evaluated here."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import encode_model as em
import rebase_model as rm
from alfalfa_amd import capi
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "encode_sim.cc")
CSRC = os.path.join(ROOT, "alfalfa_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("reencode_search.hh", "reencode_mb.hh", "rebase_inl.hh", "vp8_math.hh", "parse_common.hh", "cost_tables.h",
                                                "vp8_tables.h", "device_types.h")]
FLAGS = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]


def built(name, extra):
    out = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (out, os.getpid())             # (pytest-xdist workers may build at the same time: rename is atomic)
        subprocess.run(FLAGS + extra + [SRC, "-o", tmp], check=True)
        os.replace(tmp, out)
    return out


def sim_lib():
    L = C.CDLL(built("libencode_sim.so", ["-O2", "-fPIC", "-shared"]))
    L.encode_sim_frame.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def flat(planes):
    return np.ascontiguousarray(np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes]))


def sim_frame(L, fr):
    """One frame of encode_model.frames through the host simulation -> (mb [mbh, mbw], dense [mbh, mbw, 25, 16], recon)"""
    hdr = fr["header"]
    mbw, mbh = hdr["mb_width"], hdr["mb_height"]
    n = mbw * mbh
    target = flat(fr["target"])
    ref = flat(fr["ref"]) if fr["ref"] is not None else np.zeros(n * 384, np.uint8)
    quant = np.array(hdr["quant"][0], np.uint16)
    probs = np.ascontiguousarray(fr["mv_probs"]).reshape(-1)
    mb = np.zeros(n, capi.MB_INFO_DTYPE)
    dense = np.zeros((n, 25, 16), np.int16)
    recon = np.zeros(n * 384, np.uint8)
    assert L.encode_sim_frame(int(fr["key"]), mbw, mbh, ref.ctypes.data, target.ctypes.data, quant.ctypes.data, hdr["q_index"], probs.ctypes.data, fr["quality"],
                              mb.ctypes.data, dense.ctypes.data, recon.ctypes.data) == 0
    return mb.reshape(mbh, mbw), dense.reshape(mbh, mbw, 25, 16), recon


def differences(got_mb, got_dense, want_mb, want_dense):
    bad = []
    mbh, mbw = want_mb.shape
    for r in range(mbh):
        for c in range(mbw):
            g, w = got_mb[r, c], want_mb[r, c]
            what = [f for f in ("y_mode", "uv_mode", "ref_frame") if g[f] != w[f]]
            if (g["u"] != w["u"]).any():
                what.append("b_modes" if w["ref_frame"] == 0 else "vector %s want %s" % (rm.vectors(g)[0].tolist(), rm.vectors(w)[0].tolist()))
            if g["nz_mask"] != w["nz_mask"]:
                what.append("nz_mask %07x want %07x" % (g["nz_mask"], w["nz_mask"]))
            for b in range(25):
                if (got_dense[r, c, b] != want_dense[r, c, b]).any():
                    what.append("block %d: %s want %s" % (b, got_dense[r, c, b].tolist(), want_dense[r, c, b].tolist()))
                    break
            if what:
                bad.append("  macroblock (%d, %d) %s, got mode %d: %s" % (c, r, rm.describe(w), g["y_mode"], "; ".join(what)))
    return bad


@pytest.mark.parametrize("which", ["pred", "c0"])
@pytest.mark.parametrize("name", em.CASES)
def test_the_decision_equals_the_reference(name, which):
    L = sim_lib()
    for k, fr in enumerate(em.frames(name, which)):
        mb, dense, _ = sim_frame(L, fr)
        bad = differences(mb, dense, fr["mb"], fr["dense"])
        assert not bad, "%s %s.ivf frame %d (%s): %d of %d macroblocks differ from the reference\n%s" % (
            name, which, k, "key" if fr["key"] else "inter", len(bad), mb.size, "\n".join(bad[:8]))


def test_the_fixtures_hold_every_class_the_policies_decide():
    """Key frames: B_PRED, DC, V, H, TM and all four chroma modes; inter frames: the four inter modes, B_PRED and the four 16x16 intra
    modes, in both qualities taken together -- so an equal comparison above has met every branch."""
    key_y, key_uv, inter_y = set(), set(), {0: set(), 1: set()}
    for name, which, k in em.ALL:
        fr = em.frames(name, which)[k]
        for m in fr["mb"].reshape(-1):
            if fr["key"]:
                key_y.add(int(m["y_mode"])); key_uv.add(int(m["uv_mode"]))
            else:
                inter_y[fr["quality"]].add(int(m["y_mode"]))
    assert key_y == {0, 1, 2, 3, 4} and key_uv == {0, 1, 2, 3}, (key_y, key_uv)
    assert inter_y[0] | inter_y[1] == {0, 1, 2, 3, 4, 5, 6, 7, 8}, inter_y
    assert 4 not in inter_y[1], "B_PRED in an inter frame under -q rt"


def test_the_same_program_under_the_sanitizers(tmp_path):
    """encode_sim.cc with its own main, built with -fsanitize=address,undefined, over every fixture frame: clean, and equal to the reference."""
    exe = built("encode_sim_asan", ["-O1", "-DENCODE_SIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    files = []
    for name, which, k in em.ALL:
        fr = em.frames(name, which)[k]
        hdr = fr["header"]
        n = hdr["mb_width"] * hdr["mb_height"]
        ref = flat(fr["ref"]) if fr["ref"] is not None else np.zeros(n * 384, np.uint8)
        path = str(tmp_path / ("%s_%s_%d.case" % (name, which, k)))
        with open(path, "wb") as f:
            f.write(struct.pack("<5i", int(fr["key"]), hdr["mb_width"], hdr["mb_height"], fr["quality"], hdr["q_index"]) + np.array(hdr["quant"][0], np.uint16).tobytes()
                    + np.ascontiguousarray(fr["mv_probs"]).tobytes() + ref.tobytes() + flat(fr["target"]).tobytes()
                    + np.ascontiguousarray(fr["mb"]).tobytes() + np.ascontiguousarray(fr["dense"]).tobytes())
        files.append(path)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- the cost block's host side, against the reference's formulas as written (encoder.cc:178-193, costs.cc:135-149) ----
def y_ac_factor(q_index):
    """The luma AC factor of a quantiser index, from the product's own header maths (aa_quant_factors)."""
    return int(capi.quant_factors(q_index)[1])


def test_rd_multipliers_over_every_quantiser_index():
    L = sim_lib()
    seen = set()
    for qi in range(128):
        y_ac = y_ac_factor(qi)
        q = float(y_ac) if y_ac < 160 else 160.0
        rate = int(q * q * 2.80) & 0xFFFFFFFF            # double arithmetic, truncated to uint32_t
        if rate > 1000:
            dist, rate = 1, rate // 100
        else:
            dist = 100
        out = (C.c_uint32 * 2)()
        L.encode_sim_rd_multipliers(y_ac, out)
        assert (out[0], out[1]) == (rate, dist), "q_index %d (y_ac %d): got %s, the formula gives %s" % (qi, y_ac, (out[0], out[1]), (rate, dist))
        seen.add(dist)
    assert seen == {1, 100}, "both branches of update_rd_multipliers are met by the 128 indices"


def test_sad_costs_and_weights():
    L = sim_lib()
    got = (C.c_uint16 * 256)()
    L.encode_sim_mv_sad(got)
    want = [300] + [int(256 * (2 * float(np.log2(np.float32(8 * i))) + 0.6)) for i in range(1, 256)]      # log2f in float, the rest in double
    assert list(got) == want
    assert all(abs(want[i] - 256 * (2 * math.log2(8 * i) + 0.6)) < 1 for i in range(1, 256))
    # the weight, sad_per_bit16lut: 2 at the finest quantiser, 14 at the coarsest, never falling, runs as libvpx's table has them
    w = [L.encode_sim_sad_per_bit(qi) for qi in range(128)]
    assert w[0] == 2 and w[127] == 14 and all(b - a in (0, 1) for a, b in zip(w, w[1:]))
    assert [w.count(v) for v in range(2, 15)] == [16, 14, 12, 12, 12, 12, 12, 12, 8, 6, 6, 4, 2]


def test_key_frame_mode_costs_are_the_tree_costs_of_the_key_frame_probabilities():
    """mbmode_costs[0]: kf_y_mode_tree = {-B_PRED, 2, 4, 6, -DC, -V, -H, -TM} over kf_y_mode_probs {145, 156, 163, 128}, a bool of
    probability p costing prob_cost[p] (false) or prob_cost[255 - p] (true), as Costs::compute_cost sums them."""
    L = sim_lib()
    got = (C.c_uint16 * 5)()
    L.encode_sim_key_mode_costs(got)
    pc = (C.c_uint16 * 256)()
    L.encode_sim_prob_cost(pc)
    p = (145, 156, 163, 128)
    zero, one = (lambda q: int(pc[q])), (lambda q: int(pc[255 - q]))
    want = {4: zero(p[0]), 0: one(p[0]) + zero(p[1]) + zero(p[2]), 1: one(p[0]) + zero(p[1]) + one(p[2]),
            2: one(p[0]) + one(p[1]) + zero(p[3]), 3: one(p[0]) + one(p[1]) + one(p[3])}
    assert list(got) == [want[m] for m in range(5)]
