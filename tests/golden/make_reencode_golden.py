#!/usr/bin/env python3
"""Re-encode fixtures written by the REFERENCE (oracle/_ref/xc-enc -r = Encoder::reencode of /root/reference/src, compiled in place;
oracle/_ref/ref_state): under tests/golden/reencode/<case>/
    c0.state      the reference decoder serialised after chunk 0
    c0.ivf        chunk 0 itself: a decoder without the state format reaches the same references by decoding it
    pred.ivf      the prediction frames: chunk 1 as first encoded, key frame first
    rebased.ivf   xc-enc -r -W -q <quality> -p pred.ivf -I c0.state: frame 0 is chunk 1's key frame encoded again as an inter frame
                  predicted from c0.state (Encoder::reencode_as_interframe), frames 1.. are rebased (update_residues)
    target.yuv    raw I420, display size: every frame of chunk 1
and tests/golden/reencode/reencode_golden.json: per case the geometry, the quality and, per frame, the SHA-256 of the padded planes
the reference decodes from c0.state.  Unlike the rebase fixtures: no -e, chunk 1 starts one frame AFTER chunk 0 ends, and -q is given
to the -r run too (it decides B_PRED and how often NEWMV is searched).  Run in the build container only (needs oracle/_ref)."""
import hashlib, json, os, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_y4m, vp8_oracle as vo

REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "reencode")
#         name             w   h   n  n0 seed entropy q0  q1  quality      (chunk 0: frames 0..n0-1; chunk 1: frames n0..)
CASES = [("best_80x80",  80, 80, 5, 3, 1, "high", 100, 120, "best"),
         ("rt_80x80",    80, 80, 5, 3, 1, "high", 100, 120, "rt"),
         ("best_72x40",  72, 40, 5, 3, 1, "high", 100, 120, "best"),
         ("rt_72x40",    72, 40, 5, 3, 2, "low",   20,  30, "rt"),
         ("best_16x16",  16, 16, 5, 3, 7, "high",  30,  40, "best"),
         ("bpred_72x40", 72, 40, 5, 3, 1, "high",   4,   2, "best"),
         ("rt_low_80x80", 80, 80, 5, 3, 2, "low",  20,  30, "rt")]


def run(*cmd):
    subprocess.run(list(cmd), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def write_y4m(path, w, h, frames):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h))
        for planes in frames:
            f.write(b"FRAME\n")
            for p in planes: f.write(p.tobytes())


def main():
    out = {}
    enc = os.path.join(REF, "xc-enc")
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
            assert len(data) == fs * nf and len(vo.read_ivf(rebased)[2]) == nf
            out[name] = {"width": w, "height": h, "frames": nf, "quality": quality,
                         "raster_sha256": [hashlib.sha256(data[i * fs:(i + 1) * fs]).hexdigest() for i in range(nf)]}
            print(name, nf, "frames", sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)), "bytes")
    json.dump(out, open(os.path.join(OUT, "reencode_golden.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
