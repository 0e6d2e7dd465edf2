"""alfalfa_amd/csrc/hash_chain.hh compiled for the host (tests/cpp/hash_chain_check.cc): the walker of a job -- the source a lane of
k_hash_chains runs -- against a byte-at-a-time loop of the formula, and the segment-map job, built the way the runtime builds it,
against Parser.state_hash() (whose values tests/test_hashes.py pins to the reference's)."""
import os
import subprocess

import pytest

import alfalfa_amd as aa
from conftest import golden_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("hash_chain") / "hash_chain_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", path,
                           os.path.join(ROOT, "tests", "cpp", "hash_chain_check.cc")])
    return path


def test_job_walker_matches_the_formula_byte_by_byte(exe):
    """Lengths 0, 1, 15, 16, 17, 4 097 x source misaligned by 0..15 x seed 0 / non-zero, bytes >= 128, the 2-D form with rows of 3
    and 120 bytes, per-row pad 0 / 30, tail pad 0 / 15 x 33."""
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK ") and int(out.stdout.split()[1]) > 6 * 16 * 2 + 2 * 2 * 2 * 3 * 16 * 2


def hcombine(seed, v):
    return seed ^ ((v + 0x9e3779b9 + (seed << 6) + (seed >> 2)) & MASK)


def hrange(seed, values):
    for v in values:
        seed = hcombine(seed, int(v) & MASK)       # (signed adjustments are sign-extended to 64 bits)
    return seed


def test_segment_map_job_completes_to_the_state_hash(exe):
    """synth_33x17_s7 (3 x 2 macroblocks: map rows of 3 bytes, 30 threes behind each, 15 x 33 behind the map): on every frame with
    segmentation on, width, height and the probability tables combined on the host, the map chain walked as a job, then the filter
    adjustments -- DecoderState::hash as aa_hash_decoders_async puts it together -- equal Parser.state_hash()."""
    w, h, frames = golden_frames("synth_33x17_s7")
    p = aa.Parser(w, h)
    on = 0
    for i, fr in enumerate(frames):
        p.parse(fr)
        sg = p.segmentation()
        if not sg["enabled"]:
            continue
        on += 1
        args = [str(w), str(h), str(int(sg["absolute"]))] + [str(v) for v in sg["quant"] + sg["lf"]] + [sg["map"].tobytes().hex()]
        out = subprocess.run([exe, "segmap"] + args, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        state = hcombine(hcombine(hcombine(0, w), h), hrange(0, p.probs()))
        state = hcombine(state, int(out.stdout))
        fa = p.filter_adjustments()
        if fa["enabled"]:
            state = hcombine(state, hrange(0, fa["ref"]))
        assert state == p.state_hash(), i
    assert on >= 2
