"""Directed inter-prediction streams (tools/vp8_synth.py motion_*_stream) on the CPU: the writer's intent == what the oracle parses,
the product parser == the oracle, the oracle == the live reference byte for byte (when oracle/_ref exists), and -- the point --
the census of what the oracle parsed (tests/motion_census.py) contains EVERY class the builder promises at that size: every
sub-pel fraction and window alignment, every distance of the filter footprint to each plane edge, the compositions of the four
macroblocks one reconstruction wave carries, SPLITMV per unit.  tests/test_gpu_motion.py decodes the same streams on the GPU."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import alfalfa_amd as aa
import motion_census as mc
import vp8_oracle as vo
import vp8_synth
from conftest import GOLDEN_DIR
from parser_compare import compare
from test_synth_streams import check_intent, GPU_SEEDS, stream_of

# builder x size: the smallest frames at which the mapping cases occur (16x16: one macroblock, every non-zero vector clamps; 33x17:
# padded to 48x32; 80x48: 15 macroblocks, 4 quads, the last partial, quads straddling rows; 112x80: 35 macroblocks, 9 quads over 16
# workgroups; 144x16: one macroblock row, every macroblock touches top and bottom)
CASES = [("fraction", 112, 80), ("fraction", 80, 48),
         ("edge", 16, 16), ("edge", 33, 17), ("edge", 144, 16), ("edge", 80, 48),
         ("wave", 80, 48), ("wave", 112, 80),
         ("split", 112, 80), ("split", 16, 16), ("split", 80, 48), ("split", 144, 16)]
SEED = 1


@functools.lru_cache(maxsize=None)
def built(builder, w, h, seed=SEED):
    """One stream per session (generation is pure Python); never modified by a test."""
    return vp8_synth.MOTION_BUILDERS[builder](w, h, seed)


@functools.lru_cache(maxsize=None)
def parsed(builder, w, h, seed=SEED):
    """-> (key-frame planes, [oracle macroblocks() per frame])."""
    ora = vo.OracleDecoder(w, h)
    oms, key = [], None
    for i, fr in enumerate(built(builder, w, h, seed).frames):
        ora.decode(fr)
        if i == 0:
            key = ora.planes()
        oms.append(ora.macroblocks())
    return key, oms


def case_id(c):
    return "%s-%dx%d" % c


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_directed_stream_cpu(case, tmp_path):
    builder, w, h = case
    st = built(*case)
    assert len(st.frames) <= 13
    ref = None
    if vo.ref_available():
        path = str(tmp_path / "s.ivf"); vo.write_ivf(path, w, h, st.frames)
        vo.ref_decode(path, str(tmp_path / "s.raw"))
        ref = open(str(tmp_path / "s.raw"), "rb").read()
    pw, ph = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    fs = pw * ph * 3 // 2
    ora, par = vo.OracleDecoder(w, h), aa.Parser(w, h)
    for i, fr in enumerate(st.frames):
        ora.decode(fr)
        om = ora.macroblocks()
        check_intent(st.intent[i], om)
        hdr, mb, cf = par.parse(fr)
        compare(hdr, mb, cf, om, ora.frame_info())
        assert (par.probs() == ora.probs()).all()
        assert ora.frame_info()["loop_filter_level"] == 0
        if ref is not None:
            assert ora.raster_bytes() == ref[i * fs:(i + 1) * fs], "oracle differs from the reference at frame %d" % i
        if i == 0:
            # noisy, saturating reference planes: what makes the clamp between the two filter passes (quirk Q6) observable
            for p, plane in enumerate(ora.planes()):
                assert plane.min() == 0 and plane.max() == 255, "key frame plane %d spans %d .. %d" % (p, plane.min(), plane.max())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_census_holds_every_promised_class(case):
    builder, w, h = case
    _, oms = parsed(*case)
    present, frames = mc.stream_census(oms[1:])
    missing = sorted(mc.promised(builder, (w, h)) - present)
    assert not missing, "%s %dx%d: %d promised classes are not in the stream: %s" % (builder, w, h, len(missing), ", ".join(missing))
    if builder == "edge":
        both, whole = sum(f.edge_fractional_both for f in frames), sum(f.edge_whole_pel for f in frames)
        assert both >= whole, "border macroblocks: %d fractional in both axes, %d whole-pel" % (both, whole)
    if builder == "split":
        assert any("frame/split-only-inter" in f.classes for f in frames) and any("frame/no-split" in f.classes for f in frames)


@pytest.mark.parametrize("builder", sorted(mc.FULL))
def test_every_class_is_reached_at_some_size(builder):
    """What one size excuses another must hold: the union over sizes is the whole list, nothing excused."""
    union, promised = set(), set()
    for case in CASES:
        if case[0] == builder:
            union |= mc.stream_census(parsed(*case)[1][1:])[0]
            promised |= mc.promised(builder, case[1:])
    assert not sorted(mc.FULL[builder] - promised), "excused at every size: %s" % sorted(mc.FULL[builder] - promised)
    assert not sorted(mc.FULL[builder] - union), "reached at no size: %s" % sorted(mc.FULL[builder] - union)
    for (b, size), rules in mc.EXCUSED.items():
        assert (b,) + size in CASES and all(reason for _, reason in rules)


def test_references_differ_from_inter_frame_three_on():
    """GOLDEN and ALTREF are refreshed from different frames: a macroblock that reads the wrong reference differs."""
    w, h = 112, 80
    ora = vo.OracleDecoder(w, h)
    L = vo.lib()
    st = built("wave", w, h)
    for i, fr in enumerate(st.frames):
        if i == 3:
            refs = [np.ctypeslib.as_array(L.vp8o_ref_plane(ora.h, r, 0), shape=(80, 112)).copy() for r in (1, 2, 3)]
            assert (refs[0] != refs[1]).any() and (refs[0] != refs[2]).any() and (refs[1] != refs[2]).any()
        ora.decode(fr)
    assert len(st.frames) > 3


def test_existing_streams_are_byte_for_byte_what_they_were():
    """frame(directed=None) draws what it always drew: the hashes were taken before `directed` existed."""
    pin = json.load(open(os.path.join(GOLDEN_DIR, "synth_stream_sha256.json")))
    assert sorted(int(s) for s in pin["feature_stream"]) == list(range(100, 118)) + GPU_SEEDS
    for seed, e in sorted(pin["feature_stream"].items()):
        w, h, st = stream_of(int(seed))
        assert (w, h, len(st.frames)) == (e["width"], e["height"], e["frames"])
        assert hashlib.sha256(b"".join(st.frames)).hexdigest() == e["sha256"], "feature_stream seed %s changed" % seed
    assert len(pin["perf_stream"]) == 3
    for seed, e in sorted(pin["perf_stream"].items()):
        st = vp8_synth.perf_stream(e["width"], e["height"], int(seed), e["frames"])
        assert hashlib.sha256(b"".join(st.frames)).hexdigest() == e["sha256"], "perf_stream seed %s changed" % seed


def test_an_unreachable_directed_vector_raises():
    s = vp8_synth.SynthStream(32, 32, 1)
    s.frame(key=True)
    for mv in ((4000, 0), (0, -2050), (3, 0)):
        with pytest.raises(ValueError):
            s.frame(directed=lambda c, r: {"inter": True, "mode": vp8_synth.NEWMV, "mv": mv})
    with pytest.raises(ValueError):
        s.frame(directed=lambda c, r: {"inter": True, "mode": vp8_synth.SPLITMV, "partition": 0, "mvs": [(2, 2), (2, 5)]})


def test_oracle_chroma_vector_wrapper_is_what_the_oracle_decodes_with():
    """vp8o_stage_chroma_mv (what test_gpu_stages.py compares the device function with) against the uv_mv the whole-frame oracle
    reports, over every inter macroblock of the split streams: sums of four different vectors, both signs, and 4 x one vector."""
    import ctypes as C
    L = vo.lib()
    L.vp8o_stage_chroma_mv.restype = C.c_int; L.vp8o_stage_chroma_mv.argtypes = [C.c_int]
    seen, sums = 0, set()
    for case in CASES:
        if case[0] != "split":
            continue
        for om in parsed(*case)[1][1:]:
            for o in om.reshape(-1)[om.reshape(-1)["ref_frame"] != 0]:
                mv = o["mv"].astype(int)
                for b, g in enumerate(mc.SPLIT_GROUPS):
                    for axis in (0, 1):
                        s = int(mv[list(g), axis].sum())
                        assert L.vp8o_stage_chroma_mv(s) == int(o["uv_mv"][b][axis]), (s, o["uv_mv"][b])
                        seen += 1; sums.add(((s > 0) - (s < 0), abs(s) & 7))
    assert seen >= 500 and {(sg, r) for sg in (1, -1) for r in (0, 2, 4, 6)} <= sums


def test_the_failure_message_names_the_case():
    """explain() on a doctored raster (no GPU work): it names plane, pixel, vectors, classes, slot, the quad's others and the counts."""
    from test_gpu_motion import explain, oracle_of
    case = ("wave", 80, 48)
    want, om = oracle_of(*case)[1]
    cen = mc.FrameCensus(om)
    i = next(k for k, r in enumerate(cen.records) if r["kind"] == "whole")
    got = bytearray(want)
    got[(i // 5) * 16 * 80 + (i % 5) * 16 + 3] ^= 1
    msg = explain(bytes(got), want, om, "doctored")
    assert "1 bytes differ in 1 macroblocks; first: plane Y pixel (3, 0)" in msg and "slot %d of quad %d" % (i % 4, i // 4) in msg
    assert "chroma mv" in msg and "the rest of its quad" in msg and "all 1 differing macroblocks are" in msg and "classes: " in msg


def chance_coverage():
    """How many of the directed classes the 24 random GPU feature seeds hit by luck (reported in the pull request, not asserted)."""
    present = set()
    for seed in GPU_SEEDS:
        w, h, st = stream_of(seed)
        ora = vo.OracleDecoder(w, h)
        oms = []
        for i, fr in enumerate(st.frames):
            ora.decode(fr)
            if i:
                oms.append(ora.macroblocks())
        present |= mc.stream_census(oms)[0]
    return {b: (len(mc.FULL[b] & present), len(mc.FULL[b]), sorted(mc.FULL[b] - present)) for b in sorted(mc.FULL)}
