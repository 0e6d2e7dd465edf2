#!/usr/bin/env python3
"""Re-encode fixtures whose frame 0 carries a loop-filter level the reference SEARCHED with a real measure: make_reencode_golden.py's
recipe with every encoder run done by oracle/_ref/xc-enc-ssim -- the reference encoder with ssim() answered by the restatement of x264's
SSIM (oracle/ref_shims/ssim_restated.cc) instead of the PSNR-like stub, under which every frame 0 of tests/golden/reencode carries level
0.  Under tests/golden/lf_search/<case>/ the same five files per case (c0.state, c0.ivf, pred.ivf, rebased.ivf, target.yuv), and
tests/golden/lf_search/lf_search_golden.json: per case the geometry, the quality, the SHA-256 of the padded planes of every frame the
reference decodes from c0.state, the level in frame 0's header, and for EVERY level 0..63 of frame 0 what the search scores: the frame
rewritten with that level by the reference's serialiser (oracle/_ref/ref_rewrite), decoded by the oracle behind chunk 0, its padded luma
against the edge-extended target -- the restated SSIM as float.hex() and the integer squared error.  Run in the build container only
(needs oracle/_ref)."""
import hashlib, json, os, subprocess, sys, tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_y4m, vp8_oracle as vo
from make_reencode_golden import run, write_y4m

REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "lf_search")
#         name                 w    h   n  n0 seed entropy q0   q1  quality      (chunk 0: frames 0..n0-1; chunk 1: frames n0..)
CASES = [("ssim_best_80x80",   80,  80, 5, 3,  2, "low",  100, 120, "best"),
         ("ssim_rt_72x40",     72,  40, 5, 3,  2, "low",  110, 127, "rt"),
         ("ssim_best_176x144", 176, 144, 4, 2, 7, "low",  100, 110, "best"),
         ("ssim_rt_80x80_hi",  80,  80, 5, 3,  1, "high", 120, 127, "rt"),
         ("ssim_best_40x24",   40,  24, 5, 3, 11, "low",  110, 120, "best")]


def level_tables(td, c0_frames, frame0, w, h, target_luma):
    """-> ([SSIM as float.hex()] * 64, [luma SSE] * 64) of frame0 rewritten with every level, decoded behind chunk 0"""
    pw, ph = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    joined, var = os.path.join(td, "joined.ivf"), os.path.join(td, "var.ivf")
    vo.write_ivf(joined, w, h, c0_frames + [frame0])
    target = np.pad(target_luma, ((0, ph - h), (0, pw - w)), mode="edge")
    ssim, sse = [], []
    for level in range(64):
        run(os.path.join(REF, "ref_rewrite"), joined, var, str(level), "-1", str(len(c0_frames)))
        ora = vo.OracleDecoder(w, h)
        for fr in vo.read_ivf(var)[2]:
            ora.decode(fr)
        luma = ora.raster_bytes()[:pw * ph]
        ssim.append(float(vo.ssim_plane(luma, target.tobytes(), pw, ph)).hex())
        d = np.frombuffer(luma, np.uint8).astype(np.int64) - target.reshape(-1).astype(np.int64)
        sse.append(int((d * d).sum()))
    return ssim, sse


def main():
    out = {}
    enc = os.path.join(REF, "xc-enc-ssim")
    with tempfile.TemporaryDirectory() as td:
        for name, w, h, n, n0, seed, ent, q0, q1, quality in CASES:
            d = os.path.join(OUT, name)
            os.makedirs(d, exist_ok=True)
            c0y, c1y = os.path.join(td, "c0.y4m"), os.path.join(td, "c1.y4m")
            c0i, pred, state, rebased = (os.path.join(d, f) for f in ("c0.ivf", "pred.ivf", "c0.state", "rebased.ivf"))
            frames = list(make_y4m.synth_frames(w, h, n, seed, ent))
            chunk1 = frames[n0:]
            write_y4m(c0y, w, h, frames[:n0])
            run(enc, "-i", "y4m", "-y", str(q0), "-q", quality, "-o", c0i, c0y)
            write_y4m(c1y, w, h, chunk1)
            run(enc, "-i", "y4m", "-y", str(q1), "-q", quality, "-o", pred, c1y)
            run(os.path.join(REF, "ref_state"), "save", c0i, str(n0), state)
            run(enc, "-r", "-W", "-q", quality, "-i", "y4m", "-p", pred, "-I", state, "-o", rebased, c1y)
            with open(os.path.join(d, "target.yuv"), "wb") as f:
                for planes in chunk1:
                    for p in planes: f.write(p.tobytes())
            raw = os.path.join(td, "out.raw")
            run(os.path.join(REF, "ref_state"), "resume", rebased, "0", state, raw)
            data = open(raw, "rb").read()
            pw, ph = (w + 15) // 16 * 16, (h + 15) // 16 * 16
            fs = pw * ph * 3 // 2
            nf = len(chunk1)
            rebased_frames = vo.read_ivf(rebased)[2]
            assert len(data) == fs * nf and len(rebased_frames) == nf
            ssim, sse = level_tables(td, vo.read_ivf(c0i)[2], rebased_frames[0], w, h, np.asarray(chunk1[0][0]).reshape(h, w))
            # the level in the header of frame 0, read by the oracle: the first frame behind chunk 0
            ora = vo.OracleDecoder(w, h)
            for fr in vo.read_ivf(c0i)[2] + [rebased_frames[0]]:
                ora.decode(fr)
            assert hashlib.sha256(ora.raster_bytes()).hexdigest() == hashlib.sha256(data[:fs]).hexdigest(), name
            out[name] = {"width": w, "height": h, "frames": nf, "quality": quality,
                         "raster_sha256": [hashlib.sha256(data[i * fs:(i + 1) * fs]).hexdigest() for i in range(nf)],
                         "level": int(ora.frame_info()["loop_filter_level"]), "ssim": ssim, "sse": sse}
            print(name, nf, "frames", sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)), "bytes")
    json.dump(out, open(os.path.join(OUT, "lf_search_golden.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
