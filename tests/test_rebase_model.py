"""tests/rebase_model.py pinned to the reference, and the census of the rebase fixtures (tests/golden/rebase, written by the reference's
xc-enc -r: tests/golden/make_rebase_golden.py).  CPU only.

The model: for every whole-pel, non-split, LAST-referencing inter macroblock of the enc_* fixtures, "forward DCT of (edge-extended
target - prediction), DCs to the WHT, truncating division by the factors of the new header" gives the luma and Y2 coefficients the
reference wrote into rebased.ivf.  The references of each frame are the oracle's: chunk 0 decoded, then the rebased frames themselves
(these streams use LAST only, so the straight decode stands where c0.state does: the state's raster and the golden hashes say so).

The census: over all cases every class of macroblock the kernels treat differently is there, so a regenerated fixture cannot lose one
silently.  No macroblock is left out of either."""
import collections
import hashlib

import numpy as np
import pytest

import rebase_model as rm
import vp8_oracle as vo


@pytest.fixture(scope="module")
def cases():
    return {name: rm.load_case(name) for name in rm.CASES}


@pytest.fixture(scope="module")
def parsed(cases):
    return {name: (rm.parse_frames(c, "pred"), rm.parse_frames(c, "rebased")) for name, c in cases.items()}


@pytest.mark.parametrize("name", rm.ENC_CASES)
def test_model_reproduces_the_reference_on_whole_pel_macroblocks(cases, parsed, name):
    case = cases[name]
    pred, rebased = parsed[name]
    ora = vo.OracleDecoder(case["w"], case["h"])
    for fr in case["c0"]:
        ora.decode(fr)
    assert all((a == b).all() for a, b in zip(ora.planes(), rm.state_raster(case))), "chunk 0 decoded is not the raster of c0.state"
    checked = 0
    for k, (hdr, mb, blocks) in enumerate(rebased):
        ref_y = ora.planes()[0]
        want = rm.dense(mb, blocks)
        quant = hdr["quant"][0]
        for r in range(mb.shape[0]):
            for c in range(mb.shape[1]):
                rec = mb[r, c]
                mv = rm.vectors(rec)
                if rec["ref_frame"] != 1 or rec["y_mode"] == rm.SPLITMV or (int(mv[0][0]) & 7) or (int(mv[0][1]) & 7):
                    continue
                luma, y2 = rm.luma_of_whole_pel_macroblock(case["targets"][k][0], ref_y, c, r, (int(mv[0][0]), int(mv[0][1])), quant)
                assert luma == want[r, c, :16].tolist() and y2 == want[r, c, 24].tolist(), "%s frame %d macroblock (%d, %d): %s" % (name, k, c, r, rm.describe(rec))
                checked += 1
        ora.decode(case["rebased"][k])
        assert hashlib.sha256(ora.raster_bytes()).hexdigest() == case["sha256"][k], "%s frame %d: the oracle's decode is not the reference's" % (name, k)
    print("%s: %d whole-pel macroblocks checked, 0 differ" % (name, checked))
    assert checked > 0


def test_rebased_frames_keep_every_mode_and_vector(parsed):
    for name, (pred, rebased) in parsed.items():
        for k, (hdr, mb, _) in enumerate(rebased):
            src = pred[k + 1][1]
            for f in ("y_mode", "uv_mode", "ref_frame", "split_partition"):
                assert (mb[f] == src[f]).all(), (name, k, f)
            inter = mb["ref_frame"] != 0
            assert (mb["u"][inter] == src["u"][inter]).all(), (name, k, "vectors")
            bpred = mb["y_mode"] == rm.B_PRED
            assert (mb["u"][bpred][:, :16] == src["u"][bpred][:, :16]).all(), (name, k, "b_modes")
            assert not hdr["key_frame"] and not hdr["segmentation_enabled"], (name, k)


def test_census_of_the_fixtures(cases, parsed):
    census = collections.Counter()
    for name, (pred, rebased) in parsed.items():
        pw, ph = cases[name]["pw"], cases[name]["ph"]
        for k, (hdr, mb, blocks) in enumerate(rebased):
            for r in range(mb.shape[0]):
                for c in range(mb.shape[1]):
                    rec = mb[r, c]
                    mask = int(rec["nz_mask"])
                    if not mask:
                        census["no non-zero coefficient"] += 1
                    if (mask >> 24) and not (mask & 0xFFFF):
                        census["Y2 coded, all luma blocks zero"] += 1
                    if rec["ref_frame"] == 0:
                        census["B_PRED" if rec["y_mode"] == rm.B_PRED else "intra 16x16"] += 1
                        continue
                    if rec["ref_frame"] != 1:
                        census["reference other than LAST"] += 1
                    if rec["y_mode"] == rm.SPLITMV:
                        census["SPLITMV partition %d" % rec["split_partition"]] += 1
                        continue
                    mvx, mvy = (int(v) for v in rm.vectors(rec)[0])
                    fx, fy = mvx & 7, mvy & 7
                    census["whole-pel" if not (fx or fy) else "sub-pel in " + ("x only" if not fy else "y only" if not fx else "both")] += 1
                    # the pixels the luma prediction reads: the block at the vector, widened by the six taps where there is a fraction
                    x0, x1 = c * 16 + (mvx >> 3) - (2 if fx else 0), c * 16 + (mvx >> 3) + 15 + (3 if fx else 0)
                    y0, y1 = r * 16 + (mvy >> 3) - (2 if fy else 0), r * 16 + (mvy >> 3) + 15 + (3 if fy else 0)
                    for edge, out in (("left", x0 < 0), ("right", x1 > pw - 1), ("top", y0 < 0), ("bottom", y1 > ph - 1)):
                        if out:
                            census["window clamped at the %s edge" % edge] += 1
    print("census of tests/golden/rebase: " + ", ".join("%s: %d" % kv for kv in sorted(census.items())))
    print("Y2 coded with all luma blocks zero: %d" % census["Y2 coded, all luma blocks zero"])
    need = ["intra 16x16", "B_PRED"] + ["SPLITMV partition %d" % p for p in range(4)] + ["sub-pel in x only", "sub-pel in y only", "sub-pel in both", "whole-pel",
            "reference other than LAST", "no non-zero coefficient"] + ["window clamped at the %s edge" % e for e in ("left", "right", "top", "bottom")]
    missing = [n for n in need if not census[n]]
    assert not missing, "the fixtures hold no macroblock of: " + ", ".join(missing)


def test_quant_factors_are_the_headers(parsed):
    """aa_quant_factors from the base index alone gives the factors of every rebased header (these streams code no deltas)."""
    import alfalfa_amd as aa
    for name, (_, rebased) in parsed.items():
        for hdr, _, _ in rebased:
            assert aa.quant_factors(hdr["q_index"]) == hdr["quant"][0], (name, hdr["q_index"])
    assert aa.quant_factors(0, (0, 0, -20, 0, 0))[3] == 8 and aa.quant_factors(127, (0, 0, 0, 20, 0))[4] == 132      # the two clamps
