"""The frame-size estimate and the target-size search on the host (tests/cpp/estimate_sim.cc: reencode_search.hh under EstimateKeyPolicy and
EstimateInterPolicy, reencode_mb.hh with kSampled -- the statements the lanes of k_estimate_key / k_estimate_inter run, one lane at a time
-- estimate_size.hh's counting token walk, serializer.cpp's estimate_frame_bytes, qi_choose.hh's rule) against the reference's xc-enc:
every number a -y QI run prints as [estimated size=N], and every quantiser index a -F run chooses, over the fixtures of
tests/golden/target_size.  CPU only; the GPU run of the same comparison is tests/test_gpu_target_size.py.  The same program, stand-alone
and under AddressSanitizer / UBSan, runs over every fixture estimate.

Which frames are compared (the four pixels per macroblock row that no estimate writes are zero here and whatever a recycled raster held
in the reference): unconditionally every frame 0, every frame of a single-row small frame and every multi-row real-time inter frame
(no B_PRED trial, so no 4x4 predictor is read); a multi-row best-quality inter frame only where the host model shows its records, size
and carry independent of those pixels -- zeros, 255 and two seeded patterns give the same -- and a frame that is left out leaves out
the frames of its stream behind it, whose carry may differ.  At least half of that class must stay, and one frame of it per case."""
import struct
import subprocess

import numpy as np
import pytest

import estimate_model as em


def multi_row(case):
    return em.small_size(case["width"], case["height"])[1] > 1


def conditional(case, k):
    """The class compared only where the model shows independence of the unwritten pixels"""
    return k >= 1 and case["quality"] == "best" and multi_row(case)


_y_runs = {}


def y_run(name):
    """A -y fixture through the host model as one encoder object runs it -> [dict per frame: size, comparable, carry after]"""
    if name not in _y_runs:
        case = em.CASES[name]
        w, h, quality, q = case["width"], case["height"], case["quality"], case["q_index"]
        carry, comparable, out = em.INITIAL_CARRY, True, []
        for k, fr in enumerate(em.frames(name)):
            if fr["key"]:
                size, _ = em.sim_estimate(w, h, fr, q, quality, carry)
                out.append({"size": size, "comparable": True, "carry": carry})
                continue
            before = em.carry_in_front_of(k, carry)
            size, carry, mb, dense = em.sim_estimate(w, h, fr, q, quality, before, records=True)
            if conditional(case, k) and comparable:
                for fill in em.FILLS[1:]:
                    s2, c2, mb2, dense2 = em.sim_estimate(w, h, fr, q, quality, before, fill=fill, records=True)
                    comparable &= s2 == size and c2 == carry and mb2.tobytes() == mb.tobytes() and dense2.tobytes() == dense.tobytes()
            out.append({"size": size, "comparable": comparable, "carry": carry})
        _y_runs[name] = out
    return _y_runs[name]


@pytest.mark.parametrize("name", em.Y_CASES)
def test_every_estimate_equals_the_reference(name):
    case = em.CASES[name]
    run = y_run(name)
    for k, (got, want) in enumerate(zip(run, case["estimates"])):
        if not conditional(case, k):
            assert got["comparable"]
        if got["comparable"]:
            assert got["size"] == want, "%s frame %d: estimate %d, the reference prints %d" % (name, k, got["size"], want)
    if any(conditional(case, k) for k in range(em.FRAMES)):
        assert any(run[k]["comparable"] for k in range(em.FRAMES) if conditional(case, k)), name + ": no frame of the conditional class is left to compare"


def test_at_least_half_of_the_conditional_class_is_compared():
    total = compared = 0
    for name in em.Y_CASES:
        case = em.CASES[name]
        for k in range(em.FRAMES):
            if conditional(case, k):
                total += 1
                compared += y_run(name)[k]["comparable"]
    print("multi-row best-quality inter estimates compared with the reference: %d of %d" % (compared, total))
    assert total >= 6 and 2 * compared >= total, (compared, total)


def test_the_fixtures_keep_the_carry_path_live():
    """Some inter estimate has no intra macroblock (prob_inter is then the carry's, not its own) and some has one: both branches of
    optimize_interframe_probs are met, and the carry changes along some stream."""
    kept = replaced = 0
    for name in em.Y_CASES:
        case = em.CASES[name]
        carry = em.INITIAL_CARRY
        for k, fr in enumerate(em.frames(name)):
            if fr["key"]:
                continue
            _, after, mb, _ = em.sim_estimate(case["width"], case["height"], fr, case["q_index"], case["quality"], em.carry_in_front_of(k, carry), records=True)
            if (mb["ref_frame"] != 0).all():
                kept += 1
                assert after[0] == carry[0]
            else:
                replaced += 1
            carry = after
    assert kept and replaced, (kept, replaced)


_f_runs = {}


def f_run(name):
    """A -F fixture through the host model -> [dict per frame: q, visited, comparable, range]"""
    if name not in _f_runs:
        case = em.CASES[name]
        w, h, quality = case["width"], case["height"], case["quality"]
        carry, comparable, last_q, out = em.INITIAL_CARRY, True, None, []
        for k, fr in enumerate(em.frames(name)):
            lo, hi = em.q_range(quality, last_q)
            before = carry if fr["key"] else em.carry_in_front_of(k, carry)
            q, visited, after = em.sim_target(w, h, fr, quality, before, lo, hi, case["targets"][k])
            if conditional(case, k) and comparable:
                for fill in em.FILLS[1:]:
                    comparable &= em.sim_target(w, h, fr, quality, before, lo, hi, case["targets"][k], fill=fill) == (q, visited, after)
            if not fr["key"]:
                carry = after
            out.append({"q": q, "visited": visited, "comparable": comparable, "range": (lo, hi), "carry_before": before, "carry": after})
            last_q = case["chosen_q"][k]             # (the next frame's state is the reference's stream)
        _f_runs[name] = out
    return _f_runs[name]


@pytest.mark.parametrize("name", em.F_CASES)
def test_every_chosen_quantiser_equals_the_reference(name):
    case = em.CASES[name]
    run = f_run(name)
    for k, got in enumerate(run):
        if not conditional(case, k):
            assert got["comparable"]
        assert 1 <= len(got["visited"]) <= 7 and all(got["range"][0] <= q <= got["range"][1] for q, _ in got["visited"])
        if got["comparable"]:
            assert got["q"] == case["chosen_q"][k], "%s frame %d: chose %d after %s, the reference chose %d" % (name, k, got["q"], got["visited"], case["chosen_q"][k])
    if any(conditional(case, k) for k in range(em.FRAMES)):
        assert any(run[k]["comparable"] for k in range(em.FRAMES) if conditional(case, k)), name


def test_at_least_half_of_the_conditional_class_of_the_searches_is_compared():
    total = compared = 0
    for name in em.F_CASES:
        for k in range(em.FRAMES):
            if conditional(em.CASES[name], k):
                total += 1
                compared += f_run(name)[k]["comparable"]
    print("multi-row best-quality inter searches compared with the reference: %d of %d" % (compared, total))
    assert total >= 6 and 2 * compared >= total, (compared, total)


def test_a_picture_under_four_pixels_has_no_estimate():
    L = em.sim_lib()
    assert L.estimate_sim(1, 3, 16, None, None, 40, None, 0, None, None, 0, None, None, None) == -1


def test_the_same_program_under_the_sanitizers(tmp_path):
    """estimate_sim.cc with its own main, built with -fsanitize=address,undefined, over every estimate of every -y fixture: clean, and equal
    to the reference wherever the frame is compared."""
    exe = em.built("estimate_sim_asan", ["-O1", "-DESTIMATE_SIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    files = []
    for name in em.Y_CASES:
        case = em.CASES[name]
        run = y_run(name)
        carry = em.INITIAL_CARRY
        for k, fr in enumerate(em.frames(name)):
            before = carry if fr["key"] else em.carry_in_front_of(k, carry)
            path = str(tmp_path / ("%s_%d.case" % (name, k)))
            with open(path, "wb") as f:
                f.write(struct.pack("<6i", int(fr["key"]), case["width"], case["height"], em.QUALITY[case["quality"]], case["q_index"], 0)
                        + em.quants()[case["q_index"]].tobytes() + bytes(before) + fr["probs_before"].tobytes() + b"\0\0\0"
                        + (b"" if fr["key"] else em.flat(fr["ref"]).tobytes()) + em.flat(fr["target"]).tobytes()
                        + struct.pack("<Q", case["estimates"][k] if run[k]["comparable"] else 0))
            files.append(path)
            if not fr["key"]:
                carry = run[k]["carry"]
    out = subprocess.run([exe] + files, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stdout.count("estimate ") == len(files) == 4 * len(em.Y_CASES)
