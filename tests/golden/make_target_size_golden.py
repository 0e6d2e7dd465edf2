#!/usr/bin/env python3
"""Frame-size estimate and target-size fixtures written by the REFERENCE (oracle/_ref/xc-enc = the primary encode of /root/reference/src,
compiled in place by the committed recipe): under tests/golden/target_size/
    <case>.ivf                 the reference's output stream.  The state and the references in front of frame k are what decoding its
                               frames 0..k-1 leaves; the pictures are tools/make_y4m.synth_frames( w, h, 4, seed, entropy ), which
                               the tests regenerate (no raw video is stored)
    target_size_golden.json    per case the geometry, the generator's arguments, the quality and
        -y QI runs   "estimates": the four numbers xc-enc prints as [estimated size=N], Encoder::estimate_frame_size in front of every
                     frame, with ONE encoder object: frame 0 is a key estimate, frame 1 meets vector cost tables that are all zero,
                     frames 2..3 filled ones, and the header carry runs from each inter estimate to the next
        -F runs      "targets": the target sizes given, "chosen_q": y_ac_qi of every output frame's header (encode_with_target_size)
The targets of the -F runs are picked against the printed estimates (a target below every estimate chooses 127 everywhere, which pins
nothing).  Conditions asserted here from the reference's output alone: every -F case has a key frame and two inter frames whose chosen
index lies strictly inside its range; some real-time frame's index lies on a bound of its +-16 range; some inter frame of a -y run has
every sampled macroblock inter-coded in the stream the reference wrote (so some estimate keeps its header carry).
Run in the build container only (needs oracle/_ref and the built package)."""
import json, os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_y4m
import alfalfa_amd as aa

REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "target_size")
FRAMES = 4
#          w    h   seed entropy     (small frame; what the size covers)
CLIPS = {"16x16": (16, 16, 7, "high"),        # 1x1: one macroblock
         "72x40": (72, 40, 1, "high"),        # 2x1: the original's column 4 is the partial edge macroblock
         "336x64": (336, 64, 3, "high"),      # 6x1: a left chain; real-time NEWMV at columns 0 and 4 only
         "80x80": (80, 80, 1, "high"),        # 2x2: several rows
         "272x272": (272, 272, 2, "low")}     # 5x5: all neighbours, above-right, rows and columns under the real-time rule
LOW_QI, MID_QI = 6, 40                        # B_PRED wins often / rarely
Y_CASES = [("y_%s_%s_q%d" % (clip, quality, qi), clip, quality, qi) for clip in CLIPS for quality in ("best", "rt") for qi in (LOW_QI, MID_QI)]
#           name               clip       quality  targets
F_CASES = [("f_80x80_best",   "80x80",   "best", [4000, 1800, 3000, 1600]),
           ("f_80x80_rt",     "80x80",   "rt",   [4000, 1800, 700, 2500]),
           ("f_272x272_best", "272x272", "best", [4000, 1200, 1500, 1400]),
           ("f_272x272_rt",   "272x272", "rt",   [4000, 1200, 400, 1300]),
           ("f_336x64_rt",    "336x64",  "rt",   [6000, 2500, 5000, 1500])]


def headers_and_records(path, w, h):
    """-> [(header, mb)] of a stream, by the product's host parser"""
    _, _, frames = aa.read_ivf(path)
    p = aa.Parser(w, h)
    out = []
    for data in frames:
        hdr, mb, _ = p.parse(data)
        out.append((hdr, mb))
    return out


def q_range(quality, last_q):
    """encoder.cc:597-608, restated"""
    lo, hi = 4, 127
    if quality == "rt" and last_q is not None:
        if last_q - 16 >= lo:
            lo = last_q - 16
        hi = min(hi, last_q + 16)
    return lo, hi


def main():
    os.makedirs(OUT, exist_ok=True)
    enc = os.path.join(REF, "xc-enc")
    out = {}
    carry_kept = on_bound = False
    with tempfile.TemporaryDirectory() as td:
        clips = {}
        for clip, (w, h, seed, ent) in CLIPS.items():
            clips[clip] = os.path.join(td, clip + ".y4m")
            make_y4m.write_y4m(clips[clip], w, h, FRAMES, seed, ent)
        for name, clip, quality, qi in Y_CASES:
            w, h, seed, ent = CLIPS[clip]
            ivf = os.path.join(OUT, name + ".ivf")
            r = subprocess.run([enc, "-i", "y4m", "-y", str(qi), "-q", quality, "-o", ivf, clips[clip]], check=True, capture_output=True, text=True)
            est = [int(x) for x in re.findall(r"\[estimated size=(\d+)\]", r.stderr)]
            parsed = headers_and_records(ivf, w, h)
            assert len(est) == FRAMES and len(parsed) == FRAMES and all(hdr["q_index"] == qi for hdr, _ in parsed)
            assert parsed[0][0]["key_frame"] and not any(hdr["key_frame"] for hdr, _ in parsed[1:])
            for hdr, mb in parsed[1:]:
                carry_kept |= bool((mb[::4, ::4]["ref_frame"][:(h // 4 + 15) // 16, :(w // 4 + 15) // 16] != 0).all())
            out[name] = {"mode": "y", "width": w, "height": h, "seed": seed, "entropy": ent, "quality": quality, "q_index": qi, "estimates": est}
            print(name, est, os.path.getsize(ivf), "bytes")
        for name, clip, quality, targets in F_CASES:
            w, h, seed, ent = CLIPS[clip]
            ivf, sizes = os.path.join(OUT, name + ".ivf"), os.path.join(td, "sizes.txt")
            with open(sizes, "w") as f:
                f.write("".join("%d\n" % t for t in targets))
            subprocess.run([enc, "-i", "y4m", "-F", sizes, "-q", quality, "-o", ivf, clips[clip]], check=True, capture_output=True, text=True)
            parsed = headers_and_records(ivf, w, h)
            chosen = [hdr["q_index"] for hdr, _ in parsed]
            assert len(chosen) == FRAMES and parsed[0][0]["key_frame"] and not any(hdr["key_frame"] for hdr, _ in parsed[1:])
            inside, last = [], None
            for q in chosen:
                lo, hi = q_range(quality, last)
                assert lo <= q <= hi
                inside.append(lo < q < hi)
                on_bound |= quality == "rt" and last is not None and q in (lo, hi)
                last = q
            assert inside[0] and sum(inside[1:]) >= 2, "%s: chosen %s: the key frame and two inter frames must lie strictly inside their ranges" % (name, chosen)
            out[name] = {"mode": "F", "width": w, "height": h, "seed": seed, "entropy": ent, "quality": quality, "targets": targets, "chosen_q": chosen}
            print(name, targets, chosen, os.path.getsize(ivf), "bytes")
    assert on_bound, "no real-time frame's index lies on a bound of its +-16 range"
    assert carry_kept, "no inter frame has every sampled macroblock inter-coded: no estimate keeps its header carry"
    json.dump(out, open(os.path.join(OUT, "target_size_golden.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
