"""The fixtures of tests/golden/lf_search without a GPU -- what the reference's encoder with a real SSIM (oracle/_ref/xc-enc-ssim -r) did
with frame 0 of five chunks -- and the search rule of alfalfa_amd/csrc/lf_choose.hh against them:

  * the census: the level in frame 0's header is the one the fixture's table records; three of the five are non-zero, one is zero, one
    frame has no intra macroblock; the filter adjustments are present and zero;
  * lf_choose.hh's rule, built for the host (tests/cpp/lf_choose_check.cc as a shared library), applied to the oracle's 64 SSIM values of
    every case, in rounds of 1..8 levels, lands on the reference's level after the reference's number of candidates -- and on
    ssim_rt_72x40 over the ranges 20..22, 22..63 and 21..21;
  * on the seven fixtures of tests/golden/reencode, written under the PSNR-like stub, the rule over the squared-error measure gives level 0
    after two candidates (computed here with the oracle where oracle/_ref is built);
  * the host serialiser writes frame 0 (and every other frame) of each new rebased.ivf back byte for byte from its parsed records;
  * tests/cpp/lf_choose_check.cc itself, stand-alone under the address and undefined-behaviour sanitizers, run as a program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import alfalfa_amd as aa
import lf_search_model as lm
import rebase_model as rm
import reencode_model as rmm
import vp8_oracle as vo
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "lf_choose_check.cc")
DEPS = [SRC, os.path.join(ROOT, "alfalfa_amd", "csrc", "lf_choose.hh")]
FLAGS = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
REWRITE = os.path.join(ROOT, "oracle", "_ref", "ref_rewrite")


def built(name, extra):
    out = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (out, os.getpid())             # (pytest-xdist workers may build at the same time: rename is atomic)
        subprocess.run(FLAGS + extra + [SRC, "-o", tmp], check=True)
        os.replace(tmp, out)
    return out


def rule(scores, lo, hi, K):
    """lf_choose.hh's rule over scores[level] in rounds of K -> (best, its score, candidates consumed, rounds)"""
    L = C.CDLL(built("liblf_choose.so", ["-O2", "-fPIC", "-shared"]))
    L.lf_rule.restype = C.c_int
    arr = (C.c_double * 64)(*scores)
    best, evaluated, score = C.c_int(), C.c_int(), C.c_double()
    rounds = L.lf_rule(arr, lo, hi, K, C.byref(best), C.byref(score), C.byref(evaluated))
    return best.value, score.value, evaluated.value, rounds


# ---- the census ----
def test_the_census_of_the_new_fixtures():
    assert sorted(lm.TABLES) == sorted(lm.CASES) == sorted(lm.REFERENCE)
    levels, intra = [], []
    for name in lm.CASES:
        case = lm.load_case(name)
        p = aa.Parser(case["w"], case["h"])
        p.deserialize_state(rm.decoder_state(case))
        hdr, mb, _ = p.parse(case["rebased"][0])
        want_level, _, want_intra, want_mbs = lm.REFERENCE[name]
        assert hdr["loop_filter_level"] == want_level == lm.TABLES[name]["level"], name
        assert (int((mb["ref_frame"] == 0).sum()), mb.size) == (want_intra, want_mbs), name
        assert not hdr["key_frame"] and not hdr["segmentation_enabled"] and hdr["filter_adjustments_enabled"], name
        fa = p.filter_adjustments()
        assert fa["enabled"] and fa["ref"] == [0] * 4 and fa["mode"] == [0] * 4, (name, fa)
        ext = p.header_ext()
        assert ext["lf_delta_update"] == 1 and ext["ref_lf_update"] == [1] * 4 and ext["mode_lf_update"] == [1] * 4, name
        assert ext == aa.with_zero_lf_deltas(ext), "%s: the helper does not write what the reference wrote" % name
        assert (mb["lf_level"] == want_level).all() and (mb["segment_id"] == 0).all(), name
        assert len(lm.TABLES[name]["ssim"]) == len(lm.TABLES[name]["sse"]) == 64
        levels.append(want_level); intra.append(want_intra)
    assert sum(1 for v in levels if v) >= 3 and levels.count(0) == 1 and intra.count(0) == 1
    assert [lm.REFERENCE[n][0] for n in lm.CASES] == [1, 21, 17, 0, 16]


# ---- the rule on the oracle's tables ----
@pytest.mark.parametrize("name", lm.CASES)
def test_the_rule_lands_on_the_reference_s_level(name):
    want_level, want_evaluated, _, _ = lm.REFERENCE[name]
    scores = lm.ssim_table(name)
    for K in range(1, 9):
        best, score, evaluated, rounds = rule(scores, 0, 63, K)
        assert (best, evaluated) == (want_level, want_evaluated), (name, K)
        assert score == scores[want_level] and rounds == (want_evaluated + K - 1) // K
    assert lm.rule(scores, 0, 63) == (want_level, scores[want_level], want_evaluated)        # (the tests' own restatement agrees)


@pytest.mark.parametrize("lo,hi,want", [(20, 22, (21, 3)), (22, 63, None), (21, 21, (21, 1))])
def test_ranges_on_ssim_rt_72x40(lo, hi, want):
    scores = lm.ssim_table("ssim_rt_72x40")
    for K in range(1, 9):
        best, score, evaluated, _ = rule(scores, lo, hi, K)
        assert (best, score, evaluated) == lm.rule(scores, lo, hi)
        if want:
            assert (best, evaluated) == want
    if (lo, hi) == (22, 63):                # the scores fall from 21 on: the first candidate stays, the second ends the search
        assert lm.rule(scores, lo, hi)[0] == 22 and lm.rule(scores, lo, hi)[2] == 2


def test_the_sse_measure_is_the_stub_s_formula():
    L = C.CDLL(built("liblf_choose.so", ["-O2", "-fPIC", "-shared"]))
    L.lf_sse_score_c.restype, L.lf_sse_score_c.argtypes = C.c_double, [C.c_uint64, C.c_uint32, C.c_uint32]
    for name in lm.CASES:
        case = lm.load_case(name)
        for sse in lm.TABLES[name]["sse"]:
            assert L.lf_sse_score_c(sse, case["pw"], case["ph"]) == lm.sse_score(sse, case["pw"], case["ph"])


@pytest.mark.skipif(not os.path.exists(REWRITE), reason="oracle/_ref (the reference built in place) is not here")
@pytest.mark.parametrize("name", rmm.CASES)
def test_the_old_fixtures_stop_at_level_0_under_the_sse_measure(tmp_path, name):
    case = rmm.load_case(name)
    w, h, pw, ph = case["w"], case["h"], case["pw"], case["ph"]
    joined, var = str(tmp_path / "joined.ivf"), str(tmp_path / "var.ivf")
    vo.write_ivf(joined, w, h, case["c0"] + [case["rebased"][0]])
    target = case["targets"][0][0].astype(np.int64)
    scores = []
    for level in range(3):                  # (the rule consumes two candidates; a third shows it did not merely run out)
        subprocess.run([REWRITE, joined, var, str(level), "-1", str(len(case["c0"]))], check=True)
        ora = vo.OracleDecoder(w, h)
        for fr in vo.read_ivf(var)[2]:
            ora.decode(fr)
        d = np.frombuffer(ora.raster_bytes()[:pw * ph], np.uint8).astype(np.int64).reshape(ph, pw) - target
        scores.append(lm.sse_score(int((d * d).sum()), pw, ph))
    for K in range(1, 9):
        best, score, evaluated, _ = rule(scores + [0.0] * 61, 0, 63, K)
        assert (best, evaluated) == (0, 2) and score == scores[0], (name, K, scores)


# ---- the host serialiser on the new frames ----
@pytest.mark.parametrize("name", lm.CASES)
def test_the_reference_s_frames_are_written_again_from_their_records(name):
    from test_bool_writer import plain
    d = os.path.join(lm.GOLDEN, name)
    run = subprocess.run([plain(), os.path.join(d, "rebased.ivf") + "," + os.path.join(d, "c0.state")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    frames, same = (int(v) for v in run.stdout.split()[-3::2])
    assert frames == same == len(lm.load_case(name)["rebased"]), run.stdout


# ---- the rule's own check, stand-alone under the sanitizers ----
def test_lf_choose_check_under_the_sanitizers():
    exe = built("lf_choose_check_asan", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout, run.stdout
