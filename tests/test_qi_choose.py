"""The rule of the target-size search (alfalfa_amd/csrc/qi_choose.hh), continued one candidate at a time as aa_target_size_batch continues
it between rounds, against the plain loop of Encoder::encode_with_target_size (tests/cpp/qi_choose_check.cc: every range, targets below,
inside and above the table, falling, rising, constant, bumpy and random size tables; the starting range over every last index) -- as a
stand-alone program under AddressSanitizer / UBSan -- and a few searches followed by hand.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "qi_choose_check.cc")
DEPS = [SRC, os.path.join(ROOT, "alfalfa_amd", "csrc", "qi_choose.hh")]
FLAGS = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra"]


def built(name, extra):
    out = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (out, os.getpid())
        subprocess.run(FLAGS + extra + [SRC, "-o", tmp], check=True)
        os.replace(tmp, out)
    return out


def test_the_rule_equals_the_plain_loop_under_the_sanitizers():
    exe = built("qi_choose_check_asan", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and int(run.stdout.split()[0]) > 1000000, run.stdout


def rule(sizes, lo, hi, target):
    L = C.CDLL(built("libqi_choose.so", ["-O2", "-fPIC", "-shared"]))
    L.qi_rule.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]
    table = np.array(sizes, np.uint64)
    visited, steps = np.zeros(8, np.int32), C.c_int(0)
    best = L.qi_rule(table.ctypes.data, lo, hi, target, visited.ctypes.data, C.byref(steps))
    return best, [int(v) for v in visited[:steps.value]]


def test_searches_followed_by_hand():
    falling = [16 * (40000 // (q + 2)) for q in range(128)]
    # the whole range: seven estimates; a target nothing fits leaves the coarsest quantiser, taken by the "last candidate" clause
    assert rule(falling, 4, 127, 0) == (127, [65, 96, 112, 120, 124, 126, 127])
    # a target everything fits: the search walks down to the finest
    assert rule(falling, 4, 127, 10 ** 9) == (4, [65, 34, 18, 10, 6, 4])
    # a single candidate is taken whatever its size
    assert rule(falling, 50, 50, 0) == (50, [50])
    # the smallest index whose size fits, where the sizes fall: sizes[57] = 10832 <= 10840 < sizes[56] = 11024
    assert falling[57] == 10832 and falling[56] == 11024
    best, visited = rule(falling, 4, 127, 10840)
    assert best == 57 and visited[0] == 65 and len(visited) <= 7
    # a real-time range of +-16 around 68
    assert rule(falling, 52, 84, 0) == (84, [68, 76, 80, 82, 83, 84])
