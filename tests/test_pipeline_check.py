"""The checking pipeline (tests/pipeline_check.py) against a fake context, on the CPU: it is only worth something if it fails when a
frame is wrong, and no GPU fault is provoked to find out.  The fake's download_batch_async writes the expected bytes into the slab;
faults are put into it one at a time -- a byte flipped in a middle step (where bench.py's own check never looks), a copy that lands
after the wait that should have covered it, a delivery the context drops, a delivery the checker never sees -- and each must be
reported where it happened.  Also here: what the expected rasters are made from, and that the streams of the sub-pel GPU case
contain what that case is for."""
import ctypes as C
import hashlib
import os
import types

import numpy as np
import pytest

import pipeline_check as pc
from conftest import GOLDEN, GOLDEN_DIR

W, H = 32, 16                       # one row of two macroblocks: 32 x 16 luma, two 16 x 8 chroma planes
RASTER = 32 * 16 * 3 // 2
S, F, STEPS, RING = 4, 5, 5, 3
WHICH = [0, 1, 0, 1]                # four streams drawn from two distinct ones


class FakeDecoder:
    count = 0

    def __init__(self, ctx, w, h):
        FakeDecoder.count += 1
        self.h = types.SimpleNamespace(value=FakeDecoder.count)

    def release_before(self, n):
        pass


class FakeCtx:
    """Hand-overs and reconstruction do nothing; a download writes what the reference says the frames are -- at once, or
    (late) only at the download_wait AFTER the one that should have covered it; `flip` = (delivery, stream, offset) puts one wrong
    byte into one delivery, `drop` deliveries are accepted and never written."""

    def __init__(self, expected, flip=None, late=(), drop=()):
        self.expected, self.flip, self.late, self.drop = expected, flip, set(late), set(drop)
        self.downloads = self.waits = 0
        self.pending = []                               # (number of the wait it lands at, address, bytes)
        self.wait_args = []

    def submit_prepared(self, prepared, threads, defer, route="auto"):
        pass

    def decode_batch(self, decoders, idx):
        pass

    def launch_tokens(self, n):
        return 0

    def info(self):
        return {"memory_limit_bytes": 10 ** 12, "pool_bytes": 0, "pool_free_bytes": 0, "pool_pending_bytes": 0, "heap_mapped_bytes": 0,
                "heap_limit_bytes": 10 ** 12, "heap_used_bytes": 0, "heap_free_chunks": 0, "lanes_starved": 0, "token_workgroups_alive": 0, "jobs_waiting": 0}

    def download_wait(self, max_in_flight=None):
        self.waits += 1
        self.wait_args.append(max_in_flight)
        for p in [p for p in self.pending if p[0] <= self.waits]:
            C.memmove(p[1], p[2], len(p[2]))
            self.pending.remove(p)

    def download_batch_async(self, decoders, frame_indices, dst, stride):
        j = self.downloads
        self.downloads += 1
        assert stride == RASTER and len(decoders) == S
        data = np.concatenate([self.expected[WHICH[i]][f] for i, f in enumerate(frame_indices)])
        if self.flip and self.flip[0] == j:
            data[self.flip[1] * stride + self.flip[2]] ^= 0x10
        if j in self.drop:
            return
        if j in self.late:                              # (self.waits == j + 1 here; the wait that covers this copy is number j + 1 + RING)
            self.pending.append((self.waits + RING + 1, dst, data.tobytes()))
        else:
            C.memmove(dst, data.tobytes(), len(data))


@pytest.fixture()
def make(monkeypatch):
    import alfalfa_amd as aa
    monkeypatch.setattr(aa, "Decoder", FakeDecoder)
    rng = np.random.default_rng(20261016)
    expected = [rng.integers(0, 256, (F, RASTER), dtype=np.uint8) for _ in range(2)]
    slabs = [np.zeros(S * RASTER, np.uint8) for _ in range(RING)]

    def build(**faults):
        ctx = FakeCtx(expected, **faults)
        args = types.SimpleNamespace(trace_memory=False, overcommit=1.0, urgent_groups=2)
        env = {"ctx": ctx, "F": F, "args": args, "width": W, "height": H, "threads": 1, "distinct": [0, 1], "recon_reserve": 0, "raster_bytes": RASTER,
               "key_coeff_bytes": 1, "inter_coeff_bytes": 1, "key_arena_bytes": 1, "inter_arena_bytes": 1, "key_dense_bytes": 0,
               "urgent_keys_on_host": False, "deliver_ring": [a.ctypes.data for a in slabs]}
        streams = [[b"k%d" % i] + [b"i%d_%d" % (i, f) for f in range(1, F)] for i in range(S)]
        pipe = pc.CheckedPipeline(env, streams, 3, 2, expected=expected, which=WHICH)
        pipe.slabs = slabs                              # (the views point into these)
        return pipe, ctx
    return build


def test_a_clean_run_compares_every_raster_and_finds_nothing(make):
    pipe, ctx = make()
    pipe.run(STEPS)
    # the last RING deliveries are still in their slabs, unseen, until the end of the run is declared
    assert pipe.compared == (STEPS * F - RING) * S
    pipe.finish()
    assert pipe.mismatches == [] and pipe.bad_rasters == 0 and pipe.compared == STEPS * S * F
    pc.assert_clean_and_complete(pipe, STEPS)
    # nothing about the hand-overs changed: one wait for RING - 1 in flight before every download, as the base class issues them
    assert ctx.downloads == STEPS * F and ctx.wait_args == [RING - 1] * (STEPS * F) + [0]
    assert pipe.deliveries == STEPS * F and pipe.delivered_bytes == STEPS * F * S * RASTER
    assert pipe.decoded == STEPS and not pipe.groups
    # a second run of the same pipeline starts from empty again and is counted on
    pipe.run(2); pipe.finish()
    assert pipe.compared == (STEPS + 2) * S * F and not pipe.mismatches


@pytest.mark.parametrize("group,frame,stream,offset,where", [
    (2, 1, 3, 5 * 32 + 7, (0, 7, 5)),                               # luma
    (1, 1, 0, 32 * 16 + 3 * 16 + 9, (1, 9, 3)),                     # U
    (3, 3, 2, 32 * 16 + 16 * 8 + 7 * 16 + 15, (2, 15, 7)),          # V, its last byte
])
def test_one_wrong_byte_in_a_middle_step_is_reported_where_it_is(make, group, frame, stream, offset, where):
    """Not the last step, and not frame 0, F/2 or F-1: a fault bench.py's own check (last timed step, those three frames) cannot see."""
    assert 0 < group < STEPS - 1 and frame not in (0, F // 2, F - 1)
    pipe, ctx = make(flip=(group * F + frame, stream, offset))
    pipe.run(STEPS); pipe.finish()
    want = int(pipe.expected[WHICH[stream]][frame][offset])
    assert pipe.mismatches == [(group, frame, stream) + where + (want ^ 0x10, want)]
    assert pipe.bad_rasters == 1 and pipe.compared == STEPS * S * F and len(pipe.details) == 1
    with pytest.raises(AssertionError, match="1 rasters differ"):
        pc.assert_clean_and_complete(pipe, STEPS, "expected from a random generator")


def test_a_copy_that_lands_after_its_wait_is_reported_on_its_slab(make):
    """The copy of delivery j arrives only at the wait AFTER the one that is meant to cover it (what a download_wait that counts a
    running copy as arrived looks like from outside): when slab j % RING is looked at it still holds what it held before."""
    j = 2 * F + 1                                       # group 2, frame 1
    pipe, ctx = make(late=[j])
    pipe.run(STEPS); pipe.finish()
    assert not ctx.pending
    reported = {(g, f) for g, f, *_ in pipe.mismatches}
    assert (2, 1) in reported                           # the delivery itself: every stream of it
    assert {m[2] for m in pipe.mismatches if m[:2] == (2, 1)} == set(range(S))
    # ... and the late copy then overwrote what the next user of the slab had delivered: delivery j + RING, the same slab
    assert reported == {(2, 1), divmod(j + RING, F)} and pipe.bad_slabs == {j % RING}
    assert pipe.bad_rasters == 2 * S and pipe.compared == STEPS * S * F
    with pytest.raises(AssertionError):
        pc.assert_clean_and_complete(pipe, STEPS)


def test_a_delivery_the_context_never_wrote_is_reported(make):
    j = 1 * F + 1
    pipe, ctx = make(drop=[j])
    pipe.run(STEPS); pipe.finish()
    assert {(g, f) for g, f, *_ in pipe.mismatches} == {(1, 1)} and pipe.bad_rasters == S and pipe.compared == STEPS * S * F


def test_a_delivery_the_checker_never_saw_leaves_the_count_short(make):
    """A frame index that never reaches the delivery leg: nothing is wrong with what WAS compared, and the count says that not
    everything was."""
    pipe, ctx = make()
    real = pipe._deliver

    def deliver_but_one(ds, f):
        if (pipe.decoded, f) != (2, 1):
            real(ds, f)
    pipe._deliver = deliver_but_one
    pipe.run(STEPS); pipe.finish()
    assert pipe.mismatches == [] and pipe.compared == STEPS * S * F - S
    with pytest.raises(AssertionError, match="rasters compared"):
        pc.assert_clean_and_complete(pipe, STEPS)


def test_more_faults_than_the_report_holds_are_still_counted(make):
    pipe, ctx = make(drop=range(STEPS * F))
    pipe.run(STEPS); pipe.finish()
    assert pipe.bad_rasters == STEPS * S * F and len(pipe.mismatches) == pipe.MAX_REPORTED == len(pipe.details)


def test_locate_is_first_diffs_arithmetic():
    pw, ph = 48, 32
    assert pc.locate(0, pw, ph) == (0, 0, 0) and pc.locate(pw * ph - 1, pw, ph) == (0, pw - 1, ph - 1)
    assert pc.locate(pw * ph, pw, ph) == (1, 0, 0) and pc.locate(pw * ph + pw * ph // 4 - 1, pw, ph) == (1, pw // 2 - 1, ph // 2 - 1)
    assert pc.locate(pw * ph + pw * ph // 4 + 24 * 5 + 2, pw, ph) == (2, 2, 5)
    assert pc.padded_geometry(1920, 1080) == (1920, 1088) and pc.padded_geometry(352, 288) == (352, 288)


@pytest.mark.parametrize("name", ["qcif_q30_lf24", "cif_q60_lf40s5"])
def test_expected_rasters_are_the_stored_ones(name):
    """The helper's expected bytes for a stored stream are the rasters whose hashes the repository keeps (reference decoder and
    oracle in agreement where both are built)."""
    g = GOLDEN[name]
    n = len(g["raster_sha256"])
    (frames,), source = pc.expected_rasters([os.path.join(GOLDEN_DIR, name + ".ivf")], n, cross_check=True)
    pw, ph = pc.padded_geometry(g["width"], g["height"])
    assert frames.shape == (n, pw * ph * 3 // 2) and frames.dtype == np.uint8
    assert [hashlib.sha256(f.tobytes()).hexdigest() for f in frames] == g["raster_sha256"], source
    assert source.startswith("oracle/_ref/ref_decode") == os.path.exists(pc.REF_DECODE)


@pytest.mark.parametrize("name", ["qcif_q30_lf24", "cif_q60_lf40s5"])
def test_expected_rasters_without_the_reference_build_come_from_the_oracle(name, monkeypatch, tmp_path):
    """Where oracle/_ref/ref_decode is not built the oracle alone is the source (and says so), cross_check or not."""
    monkeypatch.setattr(pc, "REF_DECODE", str(tmp_path / "no_such_ref_decode"))
    g = GOLDEN[name]
    n = len(g["raster_sha256"])
    for cross_check in (False, True):
        (frames,), source = pc.expected_rasters([os.path.join(GOLDEN_DIR, name + ".ivf")], n, cross_check=cross_check)
        assert source.startswith("vp8_oracle.OracleDecoder") and not source.startswith("oracle/_ref/ref_decode")
        assert [hashlib.sha256(f.tobytes()).hexdigest() for f in frames] == g["raster_sha256"]


def test_the_subpel_case_contains_what_it_is_for():
    """Case b of test_gpu_pipeline_every_step.py (cif_inter_lf_subpel, 6 frames, the pool's 8 distinct streams): SPLITMV macroblocks,
    luma vectors with a fractional part in x only, in y only and in both, and predictions from all three reference frames."""
    import vp8_oracle as vo
    import workload
    paths = workload.make_streams("cif_inter_lf_subpel", 6, list(range(100, 108)), workers=pc.workers())
    split = frac_x = frac_y = frac_xy = 0
    refs, parts = set(), set()
    for p in paths:
        w, h, frames = vo.read_ivf(p)
        ora = vo.OracleDecoder(w, h)
        for fr in frames:
            ora.decode(fr)
            parts.add(ora.frame_info()["num_partitions"])
            mb = ora.macroblocks()
            inter = mb["ref_frame"] > 0
            refs.update(int(r) for r in np.unique(mb["ref_frame"][inter]))
            split += int((inter & (mb["y_mode"] == 9)).sum())
            mv = mb["mv"][inter].astype(int)                        # [macroblocks, 16 luma blocks, (x, y)], quarter-pel: & 7 is the fraction
            fx, fy = (mv[..., 0] & 7) != 0, (mv[..., 1] & 7) != 0
            frac_x += int((fx & ~fy).sum()); frac_y += int((~fx & fy).sum()); frac_xy += int((fx & fy).sum())
    assert split > 0 and frac_x > 0 and frac_y > 0 and frac_xy > 0, (split, frac_x, frac_y, frac_xy)
    assert refs == {1, 2, 3}, refs                                  # LAST, GOLDEN, ALTREF
    assert parts == {4}, parts
