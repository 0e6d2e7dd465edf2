"""The census of the re-encode fixtures (tests/golden/reencode, written by the reference: tests/golden/make_reencode_golden.py), from the
product's host parser over frame 0 of every rebased.ivf: between them the cases must hold every class the decision can produce.  A
condition on the fixtures, not a measurement: tests/test_reencode_sim.py and tests/test_gpu_reencode.py check against these frames, and
a class that is missing here is a class they do not cover.  CPU only."""
import collections
import hashlib
import os

import reencode_model as rmm

NEEDED = ["ZEROMV", "NEARESTMV", "NEARMV", "NEWMV", "intra DC", "intra V", "intra H", "intra TM", "B_PRED under -q best",
          "NEWMV on the 4x4 grid under -q rt", "sub-pel in x", "sub-pel in y", "sub-pel in x and y", "window leaves the plane"]


def test_every_class_of_the_decision_is_in_the_fixtures():
    total = collections.Counter()
    for name in rmm.CASES:
        c = rmm.census(name)
        longest = c.pop("longest vector", 0)
        total.update(c)
        total["longest vector"] = max(total["longest vector"], longest)
    for cls in NEEDED:
        assert total[cls] >= 1, "no macroblock of class '%s' in frame 0 of any fixture: %s" % (cls, dict(total))
    # vectors long enough that the prediction windows leave an 80-pixel plane altogether (80 pixels = 640 eighth-pel units is the
    # plane; a 16-pixel block whose vector exceeds 512 starts beyond the far edge's last macroblock)
    assert total["longest vector"] >= 512, total["longest vector"]


def test_the_cases_the_issue_names_are_there():
    cases = {n: rmm.load_case(n) for n in rmm.CASES}
    assert cases["best_80x80"]["quality"] == "best" and cases["rt_80x80"]["quality"] == "rt"
    same_clip = [hashlib.sha256(b"".join(p.tobytes() for p in cases[n]["targets"][0])).hexdigest() for n in ("best_80x80", "rt_80x80")]
    assert same_clip[0] == same_clip[1], "best_80x80 and rt_80x80 are one clip in both qualities"
    assert any(c["w"] % 16 or c["h"] % 16 for c in cases.values()), "one size that is no multiple of 16"
    assert (cases["best_16x16"]["pw"], cases["best_16x16"]["ph"]) == (16, 16), "the single-macroblock frame"
    c = rmm.census("bpred_72x40")
    n = (cases["bpred_72x40"]["pw"] // 16) * (cases["bpred_72x40"]["ph"] // 16)
    assert c["B_PRED under -q best"] * 2 > n, "B_PRED dominates the low-quantiser case: %d of %d" % (c["B_PRED under -q best"], n)
    for name in rmm.CASES:
        mb = rmm.parsed(name, "rebased")[0][1]
        assert rmm.parsed(name, "rebased")[0][0]["key_frame"] == 0 and rmm.parsed(name, "pred")[0][0]["key_frame"] == 1, name
        assert (mb["segment_id"] == 0).all(), name


def test_fixture_files_are_small():
    for root, _, files in os.walk(rmm.GOLDEN):
        for f in files:
            assert os.path.getsize(os.path.join(root, f)) < 64 * 1024, f
