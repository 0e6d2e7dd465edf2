"""The second pass's fixtures: the streams the reference's xc-enc -i y4m -y QI -q best|rt --two-pass wrote under tests/golden/two_pass
(tests/golden/make_two_pass_golden.py; pictures of tools/make_y4m.synth_frames) and under tests/golden/two_pass_crafted
(make_two_pass_crafted_golden.py; pictures of tools/make_y4m.crafted, which reach the three cases no synth_frames clip does) as one list of cases, each with everything a test needs: the regenerated originals, and per frame
(0: the two-pass key frame, 1: the inter frame behind it) the header, records and coefficients the product's parser reads from the
fixture's bytes, the header's token_prob_update, and the oracle's decode.  And the sweep of tests/golden/two_pass_crafted/sweep.json:
parameter tuples with the SHA-256 of the reference's key-frame records.  Test support, no product code."""
import hashlib
import json
import os
import sys

import numpy as np

import alfalfa_amd as aa
import encode_model as em
import rebase_model as rm
import vp8_oracle as vo
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_y4m  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "two_pass")
CRAFTED = os.path.join(ROOT, "tests", "golden", "two_pass_crafted")
SYNTH_META = json.load(open(os.path.join(GOLDEN, "two_pass_golden.json")))
CRAFTED_META = json.load(open(os.path.join(CRAFTED, "two_pass_crafted_golden.json")))
assert not set(SYNTH_META) & set(CRAFTED_META)
META = dict(SYNTH_META, **CRAFTED_META)
SYNTH_CASES = sorted(SYNTH_META)
CRAFTED_CASES = sorted(CRAFTED_META)
CASES = SYNTH_CASES + CRAFTED_CASES
CRAFTED_ARGS = ("family", "amp", "cell", "base", "gx", "gy", "salt")
QUALITY = {"best": 0, "rt": 1}

_cases = {}


def case(name):
    """-> dict: w, h, pw, ph, quality (0 / 1), quality_name, q_index, frames [key, inter]; a frame: header, ext, mb, blocks, dense, bytes,
    target (padded planes), mv_probs (before the frame), ref (the oracle's planes before it; None for the key frame), decoded, updates
    (the header's 1056 token_prob_update flags then its 1056 values, zero where no flag), key.  Made once."""
    if name not in _cases:
        m = META[name]
        w, h = m["width"], m["height"]
        pw, ph = (w + 15) // 16 * 16, (h + 15) // 16 * 16
        if name in CRAFTED_META:
            _, _, data = aa.read_ivf(os.path.join(CRAFTED, name + ".ivf"))
            originals = [em.pad(f, pw, ph) for f in make_y4m.crafted_frames(w, h, 2, *[m[a] for a in CRAFTED_ARGS])]
        else:
            _, _, data = aa.read_ivf(os.path.join(GOLDEN, name + ".ivf"))
            originals = [em.pad(f, pw, ph) for f in make_y4m.synth_frames(w, h, 2, m["seed"], m["entropy"])]
        p, o = aa.Parser(w, h), vo.OracleDecoder(w, h)
        frames, ref = [], None
        for k in range(2):
            probs = p.probs()[1063:1101].reshape(2, 19).copy()
            hdr, mb, blocks = p.parse(data[k])
            ext = p.header_ext()
            o.decode(data[k])
            decoded = [np.ascontiguousarray(x) for x in o.planes()]
            flags = np.array(ext["token_prob_update"], np.uint8).reshape(-1)
            values = np.where(flags != 0, np.array(ext["token_prob"], np.uint8).reshape(-1), 0).astype(np.uint8)
            frames.append({"header": hdr, "ext": ext, "mb": mb, "blocks": blocks, "dense": rm.dense(mb, blocks), "bytes": data[k], "target": originals[k],
                           "mv_probs": probs, "ref": ref, "decoded": decoded, "updates": np.concatenate([flags, values]), "key": bool(hdr["key_frame"]),
                           "quality": QUALITY[m["quality"]], "quality_name": m["quality"]})
            ref = decoded
        assert frames[0]["key"] and not frames[1]["key"] and frames[0]["header"]["q_index"] == m["q_index"]
        _cases[name] = {"w": w, "h": h, "pw": pw, "ph": ph, "quality": QUALITY[m["quality"]], "quality_name": m["quality"], "q_index": m["q_index"], "frames": frames}
    return _cases[name]


def records_digest(mb, dense):
    """SHA-256 over a key frame's records in a fixed order: per macroblock in raster order y_mode, uv_mode, the 64 u bytes, nz_mask
    (little-endian 32 bits), then its 25 x 16 dense coefficients (little-endian 16 bits)."""
    h = hashlib.sha256()
    d = np.ascontiguousarray(dense, "<i2").reshape(mb.shape[0], mb.shape[1], 400)
    for r in range(mb.shape[0]):
        for c in range(mb.shape[1]):
            m = mb[r, c]
            h.update(bytes([int(m["y_mode"]), int(m["uv_mode"])]) + np.ascontiguousarray(m["u"]).tobytes() + int(m["nz_mask"]).to_bytes(4, "little") + d[r, c].tobytes())
    return h.hexdigest()


_sweep = []


def sweep():
    """tests/golden/two_pass_crafted/sweep.json -> dict: width, height, census (the host model's sums the make script recorded), tuples
    [dict: q_index, quality, the generator's arguments, sha256 of the reference's key-frame records].  Read once."""
    if not _sweep:
        _sweep.append(json.load(open(os.path.join(CRAFTED, "sweep.json"))))
    return _sweep[0]


def sweep_target(t):
    """The padded planes of a sweep tuple's picture."""
    s = sweep()
    w, h = s["width"], s["height"]
    return em.pad(make_y4m.crafted(w, h, *[t[a] for a in CRAFTED_ARGS]), (w + 15) // 16 * 16, (h + 15) // 16 * 16)
