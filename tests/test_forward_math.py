"""The forward 4x4 DCT, the forward WHT and the quantiser of alfalfa_amd/csrc/vp8_math.hh (AA_MHD: the source the rebase kernels compile
for the device) compiled for the host by g++ (tests/cpp/forward_math_check.cc) and pinned to tests/rebase_model.py, which
tests/test_rebase_model.py pins to the reference.  Inputs: every residual block of one fixture frame (target minus the zero-motion
prediction from c0.state, all three planes) and the DCs of its macroblocks; the extremes -- all +255, all -255, the checkerboards and
stripes of +-255 --; WHT inputs at +-1020; divisions of negative and positive numerators by the factors 4, 8, 132 and 157."""
import os
import subprocess

import numpy as np
import pytest

import rebase_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("forward_math") / "forward_math_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", path, os.path.join(ROOT, "tests", "cpp", "forward_math_check.cc")])
    return path


def table():
    lines = []

    def dct(res):
        res = np.asarray(res).reshape(4, 4)
        out = rm.fdct(res)
        lines.append("D " + " ".join(str(int(v)) for v in res.reshape(-1)) + " " + " ".join(map(str, out)))
        return out

    def wht(dcs):
        lines.append("W " + " ".join(str(int(v)) for v in dcs) + " " + " ".join(map(str, rm.wht(dcs))))

    case = rm.load_case("enc_rt_64x48")
    for plane, (t, r) in enumerate(zip(case["targets"][0], rm.state_raster(case))):
        res = t.astype(np.int32) - r.astype(np.int32)
        dcs = {}
        for y in range(0, res.shape[0], 4):
            for x in range(0, res.shape[1], 4):
                c = dct(res[y:y + 4, x:x + 4])
                dcs.setdefault((y // 16, x // 16), []).append(c[0])
        if plane == 0:
            for d in dcs.values():
                wht(d)
    i = np.arange(16)
    checker, columns, rows = ((i // 4 + i % 4) % 2) * 2 - 1, (i % 2) * 2 - 1, ((i // 4) % 2) * 2 - 1
    for pattern in (np.ones(16, int), checker, columns, rows, np.where(i == 0, 1, -1), np.where(i < 8, 1, -1), np.where(i % 4 < 2, 1, -1)):
        for amp in (255, -255, 1, -1):
            dct(pattern * amp)
        for amp in (1020, -1020, 1, -1):
            wht(pattern * amp)
    wht([0] * 16)
    dct([0] * 16)
    for f in (4, 8, 132, 157):
        for n in list(range(-2 * f - 1, 2 * f + 2)) + [-32768, -20400, -8160, -4081, 4081, 8160, 20400, 32767]:
            lines.append("Q %d %d %d" % (n, f, rm.quantize([n], f, f)[0]))
    return lines


def test_vp8_math_forward_functions_equal_the_model(exe):
    lines = table()
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["OK", str(len(lines))] and len(lines) > 64 * 48 * 3 // 2 // 16
