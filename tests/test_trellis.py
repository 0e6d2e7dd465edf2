"""The second pass's quantisation (alfalfa_amd/csrc/trellis_quant.hh: trellis_quantize in the packed form k_encode_key2 runs,
check_reset_y2, the token costs of the default probabilities, coeff_base_cost) against a plain array-of-nodes restatement and the rules
the tables are computed from (tests/cpp/trellis_check.cc): a stand-alone program, built with plain g++ and again with
-fsanitize=address,undefined.  CPU only."""
import os
import subprocess

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "trellis_check.cc")
CSRC = os.path.join(ROOT, "alfalfa_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("trellis_quant.hh", "vp8_math.hh", "parse_common.hh", "cost_tables.h", "vp8_tables.h")]
FLAGS = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"]


def built(name, extra):
    out = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (out, os.getpid())             # (pytest-xdist workers may build at the same time: rename is atomic)
        subprocess.run(FLAGS + extra + [SRC, "-o", tmp], check=True)
        os.replace(tmp, out)
    return out


@pytest.mark.parametrize("name,extra", [("trellis_check", ["-O2"]),
                                        ("trellis_check_asan", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])])
def test_the_packed_trellis_equals_the_plain_one(name, extra):
    run = subprocess.run([built(name, extra)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout + run.stderr
    assert " 0 differ;" in run.stdout, run.stdout
