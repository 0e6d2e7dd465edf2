"""The size estimate's fixtures (tests/golden/target_size, written by make_target_size_golden.py from the reference's xc-enc -y QI and
-F runs) as lists of frames to estimate, each with everything a test needs -- the regenerated original, the stream's tables and the
reference frame in front of it (the product's parse and the oracle's decode of the fixture frames before it) -- and the host model
(tests/cpp/estimate_sim.cc: the kernels' statements lane by lane, the host size path, the rule of qi_choose.hh).  Test support, no
product code."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

import alfalfa_amd as aa
import vp8_oracle as vo
from alfalfa_amd import capi
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_y4m  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "target_size")
CASES = json.load(open(os.path.join(GOLDEN, "target_size_golden.json")))
Y_CASES = sorted(n for n, c in CASES.items() if c["mode"] == "y")
F_CASES = sorted(n for n, c in CASES.items() if c["mode"] == "F")
FRAMES = 4
QUALITY = {"best": 0, "rt": 1}
INITIAL_CARRY = (0, 0, 0, 0)       # a default-constructed header's three probabilities; vector cost tables not filled yet
FILLS = (0, 1, 2, 3)               # estimate_sim.cc: zeros (the product's definition), 255, two seeded patterns

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
CSRC = os.path.join(ROOT, "alfalfa_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "cpp", "estimate_sim.cc"), os.path.join(CSRC, "parser.cpp"), os.path.join(CSRC, "serializer.cpp")]
DEPS = SRC + [os.path.join(CSRC, f) for f in ("reencode_search.hh", "reencode_mb.hh", "rebase_inl.hh", "vp8_math.hh", "parse_common.hh", "cost_tables.h", "vp8_tables.h",
                                               "device_types.h", "estimate_size.hh", "qi_choose.hh", "serialize_common.hh", "bool_writer.hh", "serializer.hh", "parser.hh")]
FLAGS = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function"]


def built(name, extra):
    out = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (out, os.getpid())             # (pytest-xdist workers may build at the same time: rename is atomic)
        subprocess.run(FLAGS + extra + SRC + ["-o", tmp], check=True)
        os.replace(tmp, out)
    return out


_lib = None


def sim_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(built("libestimate_sim.so", ["-O2", "-fPIC", "-shared"]))
        _lib.estimate_sim.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
        _lib.estimate_sim_target.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def pad(planes, pw, ph):
    y, u, v = planes
    return (np.pad(y, ((0, ph - y.shape[0]), (0, pw - y.shape[1])), mode="edge"), np.pad(u, ((0, ph // 2 - u.shape[0]), (0, pw // 2 - u.shape[1])), mode="edge"),
            np.pad(v, ((0, ph // 2 - v.shape[0]), (0, pw // 2 - v.shape[1])), mode="edge"))


def flat(planes):
    return np.ascontiguousarray(np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes]))


def small_size(w, h):
    """-> (mbw_s, mbh_s) of the estimate's frame: uint16( w / 4 ) x uint16( h / 4 ) pixels"""
    return (w // 4 + 15) // 16, (h // 4 + 15) // 16


_originals = {}


def originals(w, h, seed, entropy, n=FRAMES):
    """The padded, edge-extended pictures of a clip -> [(y, u, v)]; made once"""
    key = (w, h, seed, entropy, n)
    if key not in _originals:
        pw, ph = (w + 15) // 16 * 16, (h + 15) // 16 * 16
        _originals[key] = [pad(f, pw, ph) for f in make_y4m.synth_frames(w, h, n, seed, entropy)]
    return _originals[key]


_frames = {}


def frames(name):
    """-> [dict] for the four frames of a fixture stream: key, target (padded planes of the original), probs_before (the stream's 1101 bytes
    in front of the frame), ref (the oracle's padded planes in front of it, None for frame 0), q_index (the output frame's), bytes.  Made once."""
    if name not in _frames:
        case = CASES[name]
        w, h = case["width"], case["height"]
        rw, rh, data = aa.read_ivf(os.path.join(GOLDEN, name + ".ivf"))
        assert (rw, rh) == (w, h) and len(data) == FRAMES
        pics = originals(w, h, case["seed"], case["entropy"])
        p = aa.Parser(w, h)
        o = vo.OracleDecoder(w, h)
        out, ref = [], None
        for k in range(FRAMES):
            probs = np.array(p.probs(), np.uint8).copy()
            hdr, _, _ = p.parse(data[k])
            o.decode(data[k])
            out.append({"key": bool(hdr["key_frame"]), "target": pics[k], "probs_before": probs, "ref": ref, "q_index": hdr["q_index"], "bytes": data[k]})
            ref = [np.ascontiguousarray(x) for x in o.planes()]
        assert out[0]["key"] and not any(f["key"] for f in out[1:])
        _frames[name] = out
    return _frames[name]


def q_range(quality, last_q):
    """The search's range in front of a frame: aa.target_size_range, the last index kept under real-time quality alone"""
    return aa.target_size_range(last_q if quality == "rt" else None)


_quants = None


def quants():
    global _quants
    if _quants is None:
        _quants = np.array([capi.quant_factors(q) for q in range(128)], np.uint16)
    return _quants


def sim_estimate(w, h, fr, q_index, quality, carry, fill=0, records=False):
    """One estimate by the host model -> (size, carry after) or, with records, (size, carry after, mb [mbh_s, mbw_s], dense)"""
    L = sim_lib()
    target = flat(fr["target"])
    ref = None if fr["key"] else flat(fr["ref"])
    c = np.array(carry, np.uint8)
    size = C.c_uint64(0)
    mbw, mbh = small_size(w, h)
    mb = np.zeros(mbw * mbh, capi.MB_INFO_DTYPE) if records else None
    dense = np.zeros((mbw * mbh, 25, 16), np.int16) if records else None
    rc = L.estimate_sim(int(fr["key"]), w, h, None if ref is None else ref.ctypes.data, target.ctypes.data, q_index, quants()[q_index].ctypes.data, QUALITY[quality],
                        fr["probs_before"].ctypes.data, c.ctypes.data, fill, C.byref(size), None if mb is None else mb.ctypes.data, None if dense is None else dense.ctypes.data)
    assert rc == 0
    if records:
        return size.value, tuple(int(x) for x in c), mb.reshape(mbh, mbw), dense.reshape(mbh, mbw, 25, 16)
    return size.value, tuple(int(x) for x in c)


def sim_target(w, h, fr, quality, carry, q_lo, q_hi, target_size, fill=0):
    """The search by the host model -> (chosen q, [(q, size)] visited, carry after)"""
    L = sim_lib()
    target = flat(fr["target"])
    ref = None if fr["key"] else flat(fr["ref"])
    c = np.array(carry, np.uint8)
    steps = C.c_int(0)
    vq, vs = np.zeros(8, np.int32), np.zeros(8, np.uint64)
    best = L.estimate_sim_target(int(fr["key"]), w, h, None if ref is None else ref.ctypes.data, target.ctypes.data, quants().ctypes.data, QUALITY[quality],
                                 fr["probs_before"].ctypes.data, c.ctypes.data, fill, q_lo, q_hi, int(target_size), C.byref(steps), vq.ctypes.data, vs.ctypes.data)
    assert best >= 0
    return best, [(int(vq[i]), int(vs[i])) for i in range(steps.value)], tuple(int(x) for x in c)


def carry_in_front_of(k, carry):
    """The carry an estimate of frame k (>= 1) of a stream starts from: the three probabilities as the estimate before left them; the vector
    cost tables are filled once an inter frame has been ENCODED (frame 1 meets all-zero tables)"""
    return (carry[0], carry[1], carry[2], 1 if k >= 2 else 0)
