"""The forward encoder's fixtures: the streams the reference's xc-enc -i y4m -y QI -q best|rt wrote under tests/golden/reencode --
pred.ivf (originals: target.yuv) and c0.ivf (originals: tools/make_y4m.synth_frames, regenerated and checked against target.yuv) -- as
one list of frames to encode, each with everything a test needs: the original, the header and records the product's parser reads from
the fixture's bytes, the stream's motion-vector probabilities before the frame, and the reference frame (the oracle's decode of the
fixture frames before it).  Test support, no product code."""
import os
import sys

import numpy as np

import alfalfa_amd as aa
import rebase_model as rm
import reencode_model as rmm
import vp8_oracle as vo
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_y4m  # noqa: E402

#          name          (w,  h,  n, n0, seed, entropy): tests/golden/make_reencode_golden.CASES
PARAMS = {"best_80x80": (80, 80, 5, 3, 1, "high"), "rt_80x80": (80, 80, 5, 3, 1, "high"), "best_72x40": (72, 40, 5, 3, 1, "high"),
          "rt_72x40": (72, 40, 5, 3, 2, "low"), "best_16x16": (16, 16, 5, 3, 7, "high"), "bpred_72x40": (72, 40, 5, 3, 1, "high"),
          "rt_low_80x80": (80, 80, 5, 3, 2, "low")}
CASES = rmm.CASES
STREAMS = {"pred": 2, "c0": 3}          # frames of each stream that are encoded: pred.ivf 0..1, c0.ivf 0..2
QUALITY = rmm.QUALITY


def pad(planes, pw, ph):
    y, u, v = planes
    return (np.pad(y, ((0, ph - y.shape[0]), (0, pw - y.shape[1])), mode="edge"), np.pad(u, ((0, ph // 2 - u.shape[0]), (0, pw // 2 - u.shape[1])), mode="edge"),
            np.pad(v, ((0, ph // 2 - v.shape[0]), (0, pw // 2 - v.shape[1])), mode="edge"))


_originals = {}


def originals(name, which):
    """The padded, edge-extended originals of a fixture stream's frames -> [(y, u, v)]; made once.  c0.ivf's are regenerated: the
    generator's frames n0.. must be target.yuv byte for byte, or the generator has drifted and every difference would be a false one."""
    if (name, which) not in _originals:
        case = rmm.load_case(name)
        if which == "pred":
            out = case["targets"]
        else:
            w, h, n, n0, seed, entropy = PARAMS[name]
            frames = list(make_y4m.synth_frames(w, h, n, seed, entropy))
            regenerated = b"".join(p.tobytes() for f in frames[n0:] for p in f)
            assert regenerated == open(os.path.join(rmm.GOLDEN, name, "target.yuv"), "rb").read(), \
                "%s: make_y4m.synth_frames no longer reproduces target.yuv: the originals of c0.ivf cannot be regenerated" % name
            out = [pad(f, case["pw"], case["ph"]) for f in frames[:n0]]
        _originals[name, which] = out
    return _originals[name, which]


_frames = {}


def frames(name, which):
    """-> [dict] for frames 0 .. STREAMS[which] - 1 of the stream: header, ext (header_ext), mb, blocks, dense (the product's parse of the
    fixture frame), bytes, target (padded planes), mv_probs [2][19] before the frame, ref (the oracle's padded planes before the frame, None
    in front of frame 0), decoded (the oracle's after it), quality (0 / 1), key.  Made once."""
    if (name, which) not in _frames:
        case = rmm.load_case(name)
        p = aa.Parser(case["w"], case["h"])
        o = vo.OracleDecoder(case["w"], case["h"])
        out, ref = [], None
        for k in range(STREAMS[which]):
            data = case[which][k]
            probs = p.probs()[1063:1101].reshape(2, 19).copy()
            hdr, mb, blocks = p.parse(data)
            o.decode(data)
            decoded = [np.ascontiguousarray(x) for x in o.planes()]
            assert decoded[0].shape == (case["ph"], case["pw"])
            out.append({"header": hdr, "ext": p.header_ext(), "mb": mb, "blocks": blocks, "dense": rm.dense(mb, blocks), "bytes": data,
                        "target": originals(name, which)[k], "mv_probs": probs, "ref": ref, "decoded": decoded, "quality": QUALITY[case["quality"]],
                        "quality_name": case["quality"], "key": bool(hdr["key_frame"])})
            ref = decoded
        assert out[0]["key"] and not any(f["key"] for f in out[1:])
        _frames[name, which] = out
    return _frames[name, which]


ALL = [(n, w, k) for n in CASES for w in ("pred", "c0") for k in range(STREAMS[w])]      # the 35 fixture frames


def header_like(template, width, height, q_index, key, level=0):
    """A new frame's header for a picture of another size: `template` (a parsed fixture header) with the geometry, the quantiser and the
    kind replaced."""
    from alfalfa_amd import capi
    mbw, mbh = (width + 15) // 16, (height + 15) // 16
    return dict(template, key_frame=int(key), width=width, height=height, mb_width=mbw, mb_height=mbh, num_macroblocks=mbw * mbh, q_index=q_index,
                quant=[capi.quant_factors(q_index)] * 4, loop_filter_level=level, num_coeff_blocks=0, num_intra_mbs=0)


def finished_records(mb, dense, level):
    """What the runtime makes of the decision's output (flags, nz_mask, coeff_index as the parser sets them for the serialised frame,
    lf_level = the header's, stored blocks in parse order: Y2 first) from the host simulation's (mode, vectors, raw mask, dense slots)
    -> (mb, blocks)."""
    out = mb.copy().reshape(-1)
    blocks = []
    d = dense.reshape(len(out), 25, 16)
    for i, m in enumerate(out):
        inter, has_y2 = m["ref_frame"] != 0, m["y_mode"] not in (4, 9)
        mask = int(m["nz_mask"]) & (0x1FFFFFF if has_y2 else 0xFFFFFF)
        m["flags"] = (4 if inter else 0) | (2 if has_y2 else 0) | (1 if mask else (8 | (16 if has_y2 else 0)))
        m["nz_mask"], m["coeff_index"], m["lf_level"], m["reserved"] = mask, len(blocks), level, 0
        blocks += [d[i, b] for b in [24] + list(range(24)) if (mask >> b) & 1]
    return out.reshape(mb.shape), (np.array(blocks, np.int16).reshape(-1, 16) if blocks else np.zeros((0, 16), np.int16))
