#!/usr/bin/env python3
"""Rebase fixtures written by the REFERENCE (oracle/_ref/xc-enc -r = Encoder::reencode / update_residues of
/root/reference/src, compiled in place; oracle/_ref/ref_state): under tests/golden/rebase/<case>/
    c0.state      the reference decoder serialised after chunk 0
    c0.ivf        (enc_* cases) chunk 0 itself: a decoder without the state format reaches the same references by decoding it
    pred.ivf      the prediction frames: chunk 1 as first encoded (its first frame is the key frame the rebase drops)
    rebased.ivf   xc-enc -r -e -W -p pred.ivf -I c0.state: chunk 1 without its key frame, residues recomputed against c0.state
    target.yuv    raw I420, display size: the frames the rebased frames stand for
and tests/golden/rebase/rebase_golden.json: per case the geometry and, per rebased frame, the SHA-256 of the padded planes the
reference decodes from c0.state.  Run in the build container only (needs oracle/_ref)."""
import hashlib, json, os, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_y4m, vp8_oracle as vo

REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "rebase")
#            name              w   h   n  n0 seed entropy q0   q1  quality      (chunk 0: frames 0..n0-1; chunk 1: frames n0-1..)
ENC_CASES = [("enc_rt_64x48",   64, 48, 6, 3, 11, "high", 60,  30, "rt"),
             ("enc_best_72x40", 72, 40, 6, 3,  4, "high", 35,  55, "best"),
             ("enc_skip_80x48", 80, 48, 7, 3,  2, "low",  90, 120, "best")]
#            name                 builder     w   h     (prediction: MOTION_BUILDERS[builder](w, h, 1); chunk 0: the targets' first two frames)
DIR_CASES = [("dir_split_80x48",    "split",    80, 48), ("dir_fraction_80x48", "fraction", 80, 48), ("dir_edge_80x48", "edge", 80, 48),
             ("dir_wave_80x48",     "wave",     80, 48), ("dir_split_16x16",    "split",    16, 16)]


def run(*cmd):
    subprocess.run(list(cmd), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def write_y4m(path, w, h, frames):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h))
        for planes in frames:
            f.write(b"FRAME\n")
            for p in planes: f.write(p.tobytes())


def main():
    import vp8_synth
    out = {}
    enc = os.path.join(REF, "xc-enc")
    with tempfile.TemporaryDirectory() as td:
        for case in ENC_CASES + DIR_CASES:
            name = case[0]
            w, h = case[2:4] if len(case) == 4 else case[1:3]
            d = os.path.join(OUT, name)
            os.makedirs(d, exist_ok=True)
            c0y, c1y, c0i = (os.path.join(td, f) for f in ("c0.y4m", "c1.y4m", "c0.ivf"))
            pred, state, rebased = os.path.join(d, "pred.ivf"), os.path.join(d, "c0.state"), os.path.join(d, "rebased.ivf")
            if len(case) == 4:
                stream = vp8_synth.MOTION_BUILDERS[case[1]](w, h, 1)
                vo.write_ivf(pred, w, h, stream.frames)
                frames = list(make_y4m.synth_frames(w, h, len(stream.frames), 3, "high"))
                n0, chunk1 = 2, frames
                write_y4m(c0y, w, h, frames[:2])
                run(enc, "-i", "y4m", "-y", "30", "-q", "rt", "-o", c0i, c0y)
            else:
                _, _, _, n, n0, seed, ent, q0, q1, quality = case
                frames = list(make_y4m.synth_frames(w, h, n, seed, ent))
                chunk1 = frames[n0 - 1:]
                write_y4m(c0y, w, h, frames[:n0])
                run(enc, "-i", "y4m", "-y", str(q0), "-q", quality, "-o", c0i, c0y)
                write_y4m(c1y, w, h, chunk1)
                run(enc, "-i", "y4m", "-y", str(q1), "-q", quality, "-o", pred, c1y)
                with open(c0i, "rb") as a, open(os.path.join(d, "c0.ivf"), "wb") as b: b.write(a.read())
            write_y4m(c1y, w, h, chunk1)
            run(os.path.join(REF, "ref_state"), "save", c0i, str(n0), state)
            run(enc, "-r", "-e", "-W", "-i", "y4m", "-p", pred, "-I", state, "-o", rebased, c1y)
            with open(os.path.join(d, "target.yuv"), "wb") as f:
                for planes in chunk1[1:]:
                    for p in planes: f.write(p.tobytes())
            raw = os.path.join(td, "out.raw")
            run(os.path.join(REF, "ref_state"), "resume", rebased, "0", state, raw)
            data = open(raw, "rb").read()
            pw, ph = (w + 15) // 16 * 16, (h + 15) // 16 * 16
            fs = pw * ph * 3 // 2
            nf = len(chunk1) - 1
            assert len(data) == fs * nf and len(vo.read_ivf(rebased)[2]) == nf
            out[name] = {"width": w, "height": h, "frames": nf,
                         "raster_sha256": [hashlib.sha256(data[i * fs:(i + 1) * fs]).hexdigest() for i in range(nf)]}
            print(name, nf, "frames", sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)), "bytes")
    json.dump(out, open(os.path.join(OUT, "rebase_golden.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
