"""bool_writer.hh and the host half of the serialisation without a GPU (tests/cpp/bool_writer_check.cc, a stand-alone program built here
plain and with -fsanitize=address,undefined):

  * generated (bit, probability) sequences through BoolWriter and back through bool_reader.hh's readers -- carries steered over one, two
    and more 0xff bytes, probabilities 1 and 255, the empty stream, ranges that are too small;
  * the frames the reference's Frame::serialize wrote -- every rebased.ivf of tests/golden/rebase and tests/golden/reencode, continuing
    from c0.state -- parsed by the host parser and written again from the records (first partition by serializer.cpp, DCT partitions by
    serialize_common.hh, the statements k_serialize_tokens' lanes run): the frame's bytes;
  * the same for the streams of tests/golden/serialize_fixed_point.json, and that list itself against the reference's own
    parse -> serialise where oracle/_ref is built."""
import glob
import json
import os
import subprocess
import sys

import pytest

import rebase_model as rm
import reencode_model as rmm
from conftest import GOLDEN_DIR, ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
CSRC = os.path.join(ROOT, "alfalfa_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "bool_writer_check.cc"), os.path.join(CSRC, "parser.cpp"), os.path.join(CSRC, "serializer.cpp")]
DEPS = SOURCES + [os.path.join(CSRC, f) for f in ("bool_writer.hh", "bool_reader.hh", "serialize_common.hh", "serializer.hh", "parser.hh", "parse_common.hh", "vp8_tables.h")]
FLAGS = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
FIXED = json.load(open(os.path.join(GOLDEN_DIR, "serialize_fixed_point.json")))
REF_REWRITE = os.path.join(ROOT, "oracle", "_ref", "ref_rewrite")


def built(name, extra):
    out = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (out, os.getpid())             # (pytest-xdist workers may build at the same time: rename is atomic)
        subprocess.run(FLAGS + extra + SOURCES + ["-o", tmp], check=True)
        os.replace(tmp, out)
    return out


def plain():
    return built("bool_writer_check", ["-O2"])


def sanitized():
    return built("bool_writer_check_asan", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


@pytest.mark.parametrize("exe", [plain, sanitized], ids=["plain", "sanitizers"])
def test_every_bit_written_is_read_back(exe):
    run = subprocess.run([exe()], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "carries" in run.stdout


CHUNKS = [os.path.join("rebase", n) for n in rm.CASES] + [os.path.join("reencode", n) for n in rmm.CASES]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_reference_s_frames_are_written_again_from_their_records(chunk):
    d = os.path.join(GOLDEN_DIR, chunk)
    run = subprocess.run([plain(), os.path.join(d, "rebased.ivf") + "," + os.path.join(d, "c0.state")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    frames, same = (int(v) for v in run.stdout.split()[-3::2])
    assert frames == same >= 2, run.stdout


def test_the_same_under_the_sanitizers():
    args = [os.path.join(GOLDEN_DIR, c, "rebased.ivf") + "," + os.path.join(GOLDEN_DIR, c, "c0.state") for c in CHUNKS]
    args += [os.path.join(GOLDEN_DIR, n + ".ivf") for n in FIXED["reproduced_by_reference"]]
    run = subprocess.run([sanitized()] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


@pytest.mark.parametrize("name", FIXED["reproduced_by_reference"])
def test_parse_then_serialise_is_the_identity_where_it_is_for_the_reference(name):
    run = subprocess.run([plain(), os.path.join(GOLDEN_DIR, name + ".ivf")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


def test_the_list_holds_a_loop_filter_rewrite_and_a_stream_with_inter_frames():
    names = FIXED["reproduced_by_reference"]
    assert any("_lf" in n for n in names) and any("i" in FIXED["frames"][n][2] for n in names)
    assert all(FIXED["frames"][n][0] == FIXED["frames"][n][1] for n in names)
    assert sorted(FIXED["frames"]) == sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.ivf")))


def test_frames_the_reference_does_not_reproduce_still_parse_back_the_same():
    """Streams outside the list (the synthetic ones: bytes behind the last partition, tokens a serialiser never writes): the same number
    of frames is reproduced as by the reference, and every other frame parses back to the same records (the program says so)."""
    for name, (frames, reproduced, _) in FIXED["frames"].items():
        if frames == reproduced:
            continue
        run = subprocess.run([plain(), "--list", os.path.join(GOLDEN_DIR, name + ".ivf")], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert run.stdout.split()[-3::2] == [str(frames), str(reproduced)], run.stdout
        assert run.stdout.count("parsed back: the same records") == frames - reproduced, run.stdout


@pytest.mark.skipif(not os.path.exists(REF_REWRITE), reason="the reference is not built (oracle/_ref)")
def test_the_list_is_what_the_reference_reproduces(tmp_path):
    import vp8_oracle as vo
    for name, (frames, reproduced, kinds) in FIXED["frames"].items():
        src, out = os.path.join(GOLDEN_DIR, name + ".ivf"), str(tmp_path / (name + ".ivf"))
        subprocess.run([REF_REWRITE, src, out, "-1", "-1"], check=True, capture_output=True)
        a, b = vo.read_ivf(src)[2], vo.read_ivf(out)[2]
        assert (len(a), sum(x == y for x, y in zip(a, b)), "".join("i" if f[0] & 1 else "K" for f in a)) == (frames, reproduced, kinds), name
        assert (name in FIXED["reproduced_by_reference"]) == (frames == reproduced)
