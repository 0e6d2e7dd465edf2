"""Loaders for the fixtures under tests/golden/lf_search (written by the reference with a real quality measure:
tests/golden/make_lf_search_golden.py) and the search's rule and measures restated in Python.  Test support, no product code."""
import json
import os

import numpy as np

import rebase_model as rm
import vp8_oracle as vo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lf_search")
TABLES = json.load(open(os.path.join(GOLDEN, "lf_search_golden.json")))
CASES = ["ssim_best_80x80", "ssim_rt_72x40", "ssim_best_176x144", "ssim_rt_80x80_hi", "ssim_best_40x24"]
# what the reference did with frame 0: (level in its header, candidates its search evaluated, intra macroblocks, macroblocks)
REFERENCE = {"ssim_best_80x80": (1, 3, 3, 25), "ssim_rt_72x40": (21, 23, 0, 15), "ssim_best_176x144": (17, 19, 10, 99),
             "ssim_rt_80x80_hi": (0, 2, 15, 25), "ssim_best_40x24": (16, 18, 2, 6)}

_cases, _parsed = {}, {}


def load_case(name):
    """-> dict as reencode_model.load_case gives it: w, h, pw, ph, quality, state, c0 / pred / rebased (frames), targets, sha256"""
    if name in _cases:
        return _cases[name]
    d = os.path.join(GOLDEN, name)
    g = TABLES[name]
    w, h = g["width"], g["height"]
    pw, ph = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    raw = np.fromfile(os.path.join(d, "target.yuv"), np.uint8)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    fs = w * h + 2 * cw * ch
    assert len(raw) == fs * g["frames"]
    targets = []
    for k in range(g["frames"]):
        f = raw[k * fs:(k + 1) * fs]
        y, u, v = f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:].reshape(ch, cw)
        targets.append((np.pad(y, ((0, ph - h), (0, pw - w)), mode="edge"), np.pad(u, ((0, ph // 2 - ch), (0, pw // 2 - cw)), mode="edge"),
                        np.pad(v, ((0, ph // 2 - ch), (0, pw // 2 - cw)), mode="edge")))
    case = {"name": name, "w": w, "h": h, "pw": pw, "ph": ph, "quality": g["quality"], "state": open(os.path.join(d, "c0.state"), "rb").read(),
            "c0": vo.read_ivf(os.path.join(d, "c0.ivf"))[2], "pred": vo.read_ivf(os.path.join(d, "pred.ivf"))[2],
            "rebased": vo.read_ivf(os.path.join(d, "rebased.ivf"))[2], "targets": targets, "sha256": g["raster_sha256"]}
    assert len(case["pred"]) == len(case["rebased"]) == g["frames"]
    _cases[name] = case
    return case


def parsed(name):
    """The product's host parser over rebased.ivf, continuing from c0.state -> [(header, mb, blocks)]; made once."""
    if name not in _parsed:
        _parsed[name] = rm.parse_frames(load_case(name), "rebased")
    return _parsed[name]


def ssim_table(name):
    return [float.fromhex(x) for x in TABLES[name]["ssim"]]


def sse_score(sse, pw, ph):
    """oracle/ref_shims/ssim_stub.cc's value from the integer squared error of a pw x ph plane, in double precision, that grouping"""
    return 1.0 - (float(sse) / (float(pw) * float(ph))) / (255.0 * 255.0)


def sse_table(name):
    case = load_case(name)
    return [sse_score(s, case["pw"], case["ph"]) for s in TABLES[name]["sse"]]


def rule(scores, lo, hi):
    """choose_level's rule over scores[level] -> (best level, its score, candidates consumed)"""
    best, best_q, evaluated = lo, -1.0, 0
    for level in range(lo, hi + 1):
        evaluated += 1
        if scores[level] > best_q:
            best, best_q = level, scores[level]
        else:
            break
    return best, best_q, evaluated
