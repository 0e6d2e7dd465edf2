"""Loaders and the census of the fixtures under tests/golden/reencode (written by the reference: tests/golden/make_reencode_golden.py).
Test support, no product code.  Frame 0 of rebased.ivf is the chunk's key frame encoded again as an inter frame
(Encoder::reencode_as_interframe); frames 1.. are rebased inter frames."""
import collections
import json
import os

import numpy as np

import alfalfa_amd as aa
import rebase_model as rm
import vp8_oracle as vo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reencode")
HASHES = json.load(open(os.path.join(GOLDEN, "reencode_golden.json")))
CASES = ["best_80x80", "rt_80x80", "best_72x40", "rt_72x40", "best_16x16", "bpred_72x40", "rt_low_80x80"]
QUALITY = {"best": 0, "rt": 1}
DC_PRED, V_PRED, H_PRED, TM_PRED, B_PRED, NEARESTMV, NEARMV, ZEROMV, NEWMV, SPLITMV = range(10)

_cases = {}


def load_case(name):
    """-> dict: w, h, pw, ph, quality, state (bytes), c0 / pred / rebased (frames), targets ([(y, u, v)] padded and edge-extended),
    sha256 ([hex]); made once."""
    if name in _cases:
        return _cases[name]
    d = os.path.join(GOLDEN, name)
    g = HASHES[name]
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


_parsed = {}


def parsed(name, which):
    """The product's host parser over pred.ivf or rebased.ivf (continuing from c0.state) -> [(header, mb, blocks)]; made once."""
    if (name, which) not in _parsed:
        _parsed[name, which] = rm.parse_frames(load_case(name), which)
    return _parsed[name, which]


def mv_probs(name):
    """The motion-vector probabilities the stream holds after chunk 0 -- what the costs of frame 0's vectors are built from -- as
    [2][19] (row, column), read by the product's parser from c0.ivf."""
    case = load_case(name)
    p = aa.Parser(case["w"], case["h"])
    p.deserialize_state(rm.decoder_state(case))
    return p.probs()[1063:1101].reshape(2, 19).copy()


def census(name):
    """Frame 0 of rebased.ivf by class -> Counter."""
    _, mb, _ = parsed(name, "rebased")[0]
    quality = load_case(name)["quality"]
    c = collections.Counter()
    mbh, mbw = mb.shape
    for r in range(mbh):
        for col in range(mbw):
            m = mb[r, col]
            y = int(m["y_mode"])
            if m["ref_frame"] == 0:
                c[("intra DC", "intra V", "intra H", "intra TM", "B_PRED under -q " + quality)[y]] += 1
                continue
            assert m["ref_frame"] == 1 and y != SPLITMV, "the re-encode predicts whole macroblocks from LAST only"
            c[{NEARESTMV: "NEARESTMV", NEARMV: "NEARMV", ZEROMV: "ZEROMV", NEWMV: "NEWMV"}[y]] += 1
            x, yv = (int(v) for v in rm.vectors(m)[0])
            if y == NEWMV and quality == "rt":
                assert col % 4 == 0 and r % 4 == 0, "NEWMV off the 4x4 grid under -q rt"
                c["NEWMV on the 4x4 grid under -q rt"] += 1
            if x & 7 and yv & 7: c["sub-pel in x and y"] += 1
            elif x & 7: c["sub-pel in x"] += 1
            elif yv & 7: c["sub-pel in y"] += 1
            # the 9x9 window of a luma unit leaves the plane
            x0, y0 = col * 16 + (x >> 3), r * 16 + (yv >> 3)
            if x0 - 2 < 0 or y0 - 2 < 0 or x0 + 16 + 3 > mbw * 16 or y0 + 16 + 3 > mbh * 16:
                c["window leaves the plane"] += 1
            c["longest vector"] = max(c["longest vector"], abs(x), abs(yv))
    return c
