#!/usr/bin/env python3
"""Second-pass fixtures for the three cases no clip of tools/make_y4m.synth_frames reaches -- a Y2 block emptied by check_reset_y2, B_PRED
chosen in the second pass after a 16x16 mode of the first, a first-pass Y2 flag that is SET under a macroblock that is B_PRED in the
second pass -- written by the REFERENCE (oracle/_ref/xc-enc, compiled in place by the committed recipe; nothing else of the reference is
read) over the pictures of tools/make_y4m.crafted, which the tests regenerate: under tests/golden/two_pass_crafted/
    <case>.ivf                     xc-enc -i y4m -y QI -q best|rt --two-pass over a two-frame clip of one crafted 64x64 picture: the key
                                   frame in two passes and the inter frame behind it
    two_pass_crafted_golden.json   per case the geometry, the generator's arguments, the quality and the index
    sweep.json                     SWEEP parameter tuples found by a seeded hunt (random tuples, every other one faint and at a low index;
                                   those kept whose host-model census meets one of the three cases), qualities alternating best / rt; per tuple the SHA-256
                                   (tests/two_pass_model.records_digest) of the key-frame records the product's parser reads from the
                                   reference's output; and the host model's census sums over the sweep
Asserted here, and nothing is written otherwise: the host model (tests/cpp/encode2_sim.cc) equals the reference's records on EVERY case and
EVERY sweep tuple; every case's key frame differs from its one-pass twin; from the host model's census Y2_RESET > 0 in at least two cases,
one of them -q rt, BPRED_AFTER_16X16 > 0 in at least three cases at an index below 20, between 20 and 60 and above 100, STALE_Y2_SET > 0 in
at least two cases; over the sweep at least 100 Y2 resets, 30 B_PRED-after-16x16 and 20 set stale flags.
Run in the build container only (needs oracle/_ref and the built package)."""
import json, os, subprocess, sys, tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
sys.dont_write_bytecode = True
OUT = os.path.join(HERE, "two_pass_crafted")
os.makedirs(OUT, exist_ok=True)
if not os.path.exists(os.path.join(OUT, "two_pass_crafted_golden.json")):          # (tests/two_pass_model.py reads it on import)
    json.dump({}, open(os.path.join(OUT, "two_pass_crafted_golden.json"), "w"))
import make_y4m
import alfalfa_amd as aa
import encode_model as em
import rebase_model as rm
import two_pass_model as tp
import test_encode2_sim as sim
from test_encode_sim import differences

ENC = os.path.join(ROOT, "oracle", "_ref", "xc-enc")
W = H = 64
ARGS = tp.CRAFTED_ARGS
#         name               quality  index  family    amp cell base gx gy salt
CASES = [("sparse_q11",      "best",  11,   "sparse",   14, 8, 131, 4, 0, 1121),
         ("sparse_q2",       "best",  2,    "sparse",    7, 4, 107, 2, 4,  783),
         ("checker_rt_q2",   "rt",    2,    "checker",   1, 1, 127, 4, 0, 1196),
         ("checker_q126",    "best",  126,  "checker", 125, 4,  67, 2, 0,  116),
         ("dot_rt_q26",      "rt",    26,   "dot",      24, 8, 115, 0, 1,  792),
         ("dot_q40",         "best",  40,   "dot",      23, 8,  45, 0, 1, 1325),
         ("sparse_q0",       "best",  0,    "sparse",    1, 1, 138, 2, 2,  914),
         ("sparse_rt_q9",    "rt",    9,    "sparse",    8, 4, 144, 0, 3, 1332)]
SWEEP, HUNT_SEED = 112, 20240917
FLOORS = {"Y2_RESET": 100, "BPRED_AFTER_16X16": 30, "STALE_Y2_SET": 20}
WORDS = {"Y2_RESET": sim.Y2_RESET, "BPRED_AFTER_16X16": sim.BPRED_AFTER_16X16, "STALE_Y2_SET": sim.STALE_Y2_SET}


def reference(td, quality, qi, args, frames, keep=None, one_pass=False):
    """xc-enc over `frames` copies of the crafted picture -> the frames of its output"""
    clip, ivf = os.path.join(td, "clip.y4m"), keep or os.path.join(td, "out.ivf")
    make_y4m.write_y4m_frames(clip, W, H, make_y4m.crafted_frames(W, H, frames, *args))
    subprocess.run([ENC, "-i", "y4m", "-y", str(qi), "-q", quality] + ([] if one_pass else ["--two-pass"]) + ["-o", ivf, clip], check=True, capture_output=True, text=True)
    out = aa.read_ivf(ivf)[2]
    assert len(out) == frames
    return out


def host_model(L, template, qi, args):
    hdr = em.header_like(template, W, H, qi, key=True)
    return sim.sim_two_pass(L, hdr, em.pad(make_y4m.crafted(W, H, *args), W, H))


def against_the_reference(label, L, template, qi, args, key_frame):
    """The host model against the parse of the reference's key frame: equal, or nothing is written -> (digest, census)"""
    hdr, mb, blocks = aa.Parser(W, H).parse(key_frame)
    assert hdr["key_frame"] and hdr["q_index"] == qi
    dense = rm.dense(mb, blocks)
    smb, sdense, _, _, _, census = host_model(L, template, qi, args)
    bad = differences(smb, sdense, mb, dense)
    assert not bad, "%s: the host model differs from the reference\n%s" % (label, "\n".join(bad[:8]))
    digest = tp.records_digest(mb, dense)
    assert tp.records_digest(smb, sdense) == digest, label
    return digest, census


def main():
    L = sim.sim_lib()
    template = tp.case(tp.SYNTH_CASES[0])["frames"][0]["header"]
    with tempfile.TemporaryDirectory() as td:
        # ---- the cases ----
        meta, met = {}, {}
        for name, quality, qi, *args in CASES:
            two = reference(td, quality, qi, args, 2, keep=os.path.join(OUT, name + ".ivf"))
            one = reference(td, quality, qi, args, 2, one_pass=True)
            assert two[0] != one[0], "%s: the second pass changes nothing in the key frame: the case pins nothing" % name
            _, census = against_the_reference(name, L, template, qi, args, two[0])
            met[name] = {k: int(census[i]) for k, i in WORDS.items()}
            meta[name] = dict(zip(ARGS, args), width=W, height=H, quality=quality, q_index=qi, check_reset_y2=bool(met[name]["Y2_RESET"]), census=met[name])
            print(name, [len(x) for x in two], met[name])
        resets = [n for n in meta if met[n]["Y2_RESET"]]
        after = [meta[n]["q_index"] for n in meta if met[n]["BPRED_AFTER_16X16"]]
        assert len(resets) >= 2 and any(meta[n]["quality"] == "rt" for n in resets), resets
        assert len(after) >= 3 and any(q < 20 for q in after) and any(20 <= q <= 60 for q in after) and any(q > 100 for q in after), after
        assert sum(1 for n in meta if met[n]["STALE_Y2_SET"]) >= 2
        # ---- the sweep: a seeded hunt over the host model, then every tuple kept goes through the reference ----
        rng = np.random.default_rng(HUNT_SEED)
        tuples, total, tried = [], {k: 0 for k in WORDS}, 0
        while len(tuples) < SWEEP:
            tried += 1
            low = tried % 2 == 0                               # (check_reset_y2 acts at low indices only, on faint pictures: every other try is one)
            family = make_y4m.CRAFTED_FAMILIES[int(rng.integers(4))]
            args = [family, int(rng.integers(1, 10 if low else 128)), int(2 ** rng.integers(4)), int(rng.integers(16, 200)), int(rng.integers(5)), int(rng.integers(5)), int(rng.integers(2000))]
            qi = int(rng.integers(30 if low else 128))
            census = host_model(L, template, qi, args)[5]
            if not any(census[i] for i in WORDS.values()):
                continue
            quality = ("best", "rt")[len(tuples) % 2]
            digest, census2 = against_the_reference("sweep tuple %d %s" % (len(tuples), [qi, quality] + args), L, template, qi, args, reference(td, quality, qi, args, 1)[0])
            assert (census2 == census).all()
            for k, i in WORDS.items():
                total[k] += int(census[i])
            tuples.append(dict(zip(ARGS, args), q_index=qi, quality=quality, sha256=digest))
        print("sweep: %d tuples of %d tried, census %s" % (len(tuples), tried, total))
        assert all(total[k] >= FLOORS[k] for k in FLOORS), "the sweep's census %s is below %s" % (total, FLOORS)
    json.dump(meta, open(os.path.join(OUT, "two_pass_crafted_golden.json"), "w"), indent=1, sort_keys=True)
    json.dump({"width": W, "height": H, "hunt_seed": HUNT_SEED, "tried": tried, "census": total, "tuples": tuples}, open(os.path.join(OUT, "sweep.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
