"""The re-encode's decision on the host (tests/cpp/reencode_sim.cc: reencode_search.hh, reencode_mb.hh and rebase_inl.hh, the statements
k_reencode_inter's lanes run, one lane at a time) against the reference's xc-enc -r on the fixtures of tests/golden/reencode: every
mode, vector, b_mode and uv_mode and every coefficient of frame 0 of every fixture.  CPU only; the GPU run of the same comparison is
tests/test_gpu_reencode.py.  The same program, stand-alone and under AddressSanitizer / UBSan, runs over the same inputs."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import rebase_model as rm
import reencode_model as rmm
from alfalfa_amd import capi
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "reencode_sim.cc")
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


def inputs(name):
    """-> (mbw, mbh, reference planes, target planes, quant[6], mv_probs[38], quality, the reference's records, its dense coefficients)"""
    case = rmm.load_case(name)
    hdr, want_mb, want_blocks = rmm.parsed(name, "rebased")[0]
    ref = np.concatenate([p.reshape(-1) for p in rm.state_raster(case)])
    target = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in case["targets"][0]])
    quant = np.array(hdr["quant"][0], np.uint16)
    return (hdr["mb_width"], hdr["mb_height"], np.ascontiguousarray(ref), np.ascontiguousarray(target), quant, np.ascontiguousarray(rmm.mv_probs(name)).reshape(-1),
            rmm.QUALITY[case["quality"]], want_mb, rm.dense(want_mb, want_blocks))


@pytest.mark.parametrize("name", rmm.CASES)
def test_the_decision_equals_the_reference(name):
    L = C.CDLL(built("libreencode_sim.so", ["-O2", "-fPIC", "-shared"]))
    mbw, mbh, ref, target, quant, probs, quality, want_mb, want_dense = inputs(name)
    n = mbw * mbh
    mb = np.zeros(n, capi.MB_INFO_DTYPE)
    dense = np.zeros((n, 25, 16), np.int16)
    recon = np.zeros(n * 384, np.uint8)
    L.reencode_sim_frame.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3
    assert L.reencode_sim_frame(mbw, mbh, ref.ctypes.data, target.ctypes.data, quant.ctypes.data, probs.ctypes.data, quality, mb.ctypes.data,
                                dense.ctypes.data, recon.ctypes.data) == 0
    mb, dense = mb.reshape(mbh, mbw), dense.reshape(mbh, mbw, 25, 16)
    bad = []
    for r in range(mbh):
        for c in range(mbw):
            g, w = mb[r, c], want_mb[r, c]
            what = [f for f in ("y_mode", "uv_mode", "ref_frame") if g[f] != w[f]]
            if (g["u"] != w["u"]).any():
                what.append("b_modes" if w["ref_frame"] == 0 else "vector %s want %s" % (rm.vectors(g)[0].tolist(), rm.vectors(w)[0].tolist()))
            if g["nz_mask"] != w["nz_mask"]:
                what.append("nz_mask %07x want %07x" % (g["nz_mask"], w["nz_mask"]))
            for b in range(25):
                if (dense[r, c, b] != want_dense[r, c, b]).any():
                    what.append("block %d: %s want %s" % (b, dense[r, c, b].tolist(), want_dense[r, c, b].tolist()))
                    break
            if what:
                bad.append("  macroblock (%d, %d) %s, got mode %d: %s" % (c, r, rm.describe(w), g["y_mode"], "; ".join(what)))
    assert not bad, "%s: %d of %d macroblocks differ from the reference\n%s" % (name, len(bad), n, "\n".join(bad[:8]))


def test_the_same_program_under_the_sanitizers(tmp_path):
    """reencode_sim.cc with its own main, built with -fsanitize=address,undefined, over every fixture: clean, and equal to the reference."""
    exe = built("reencode_sim_asan", ["-O1", "-DREENCODE_SIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    files = []
    for name in rmm.CASES:
        mbw, mbh, ref, target, quant, probs, quality, want_mb, want_dense = inputs(name)
        path = str(tmp_path / (name + ".case"))
        with open(path, "wb") as f:
            f.write(struct.pack("<3i", mbw, mbh, quality) + quant.tobytes() + probs.tobytes() + ref.tobytes() + target.tobytes()
                    + np.ascontiguousarray(want_mb).tobytes() + np.ascontiguousarray(want_dense).tobytes())
        files.append(path)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
