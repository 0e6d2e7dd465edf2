"""Directed inter-prediction parity (needs a real MI355X): the streams of tools/vp8_synth.py's motion_*_stream builders -- every
sub-pel fraction and window alignment, every distance of the filter footprint to each plane edge, the compositions of the four
macroblocks one reconstruction wave carries, SPLITMV per unit -- decoded through the C ABI and compared with the oracle: every
byte of all three padded planes of every frame, bit-exact.  tests/test_motion_streams.py shows on the CPU that the same streams
(same builders, sizes and seeds) are oracle == live reference byte for byte and that their census holds every promised class,
so HIP == oracle here is HIP == reference on exactly those cases.  A difference is reported by CASE: the first differing
macroblock with its vectors, fractions, distances, slot and quad, and how many macroblocks of each class differ."""
import collections

import numpy as np
import pytest

import alfalfa_amd as aa
import motion_census as mc
import vp8_oracle as vo
from test_motion_streams import CASES, SEED, built, case_id

pytestmark = pytest.mark.gpu


def explain(got, want, om, label):
    """The message for a differing frame: planes are the padded Y, U, V of an mbw x mbh frame, concatenated."""
    mbh, mbw = om.shape
    pw, ph = mbw * 16, mbh * 16
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if len(a) != len(b):
        return "%s: %d bytes, want %d" % (label, len(a), len(b))
    diff = a != b
    planes, off = [], 0
    for name, w, h, n in (("Y", pw, ph, 16), ("U", pw // 2, ph // 2, 8), ("V", pw // 2, ph // 2, 8)):
        planes.append((name, n, diff[off:off + w * h].reshape(h, w), a[off:off + w * h].reshape(h, w), b[off:off + w * h].reshape(h, w)))
        off += w * h
    bad = {}          # macroblock index -> (plane, x, y, got, want) of its first differing pixel
    for name, n, d, ga, wa in planes:
        for y, x in zip(*np.nonzero(d)):
            i = int(y // n) * mbw + int(x // n)
            if i not in bad:
                bad[i] = (name, int(x % n), int(y % n), int(ga[y, x]), int(wa[y, x]))
    cen = mc.FrameCensus(om)
    first = min(bad)
    pl, x, y, g, w = bad[first]
    lines = ["%s: %d bytes differ in %d macroblocks; first: plane %s pixel (%d, %d) of the macroblock, got %d want %d" % (label, int(diff.sum()), len(bad), pl, x, y, g, w),
             "  " + cen.describe(first), "  classes: " + ", ".join(sorted(cen.macroblock_classes(first))), "  the rest of its quad:"]
    lines += ["    " + cen.describe(i) for i in range(4 * (first // 4), min(4 * (first // 4) + 4, mbw * mbh)) if i != first]
    counts = collections.Counter(cen.summary(i) for i in bad)
    if len(counts) == 1:
        lines.append("  all %d differing macroblocks are %s" % (len(bad), next(iter(counts))))
    else:
        lines += ["  %d differing macroblocks are %s" % (n, c) for c, n in counts.most_common()]
    return "\n".join(lines)


def oracle_frames(st, w, h):
    """-> [(raster bytes, macroblocks())] of every frame."""
    ora = vo.OracleDecoder(w, h)
    out = []
    for fr in st.frames:
        ora.decode(fr)
        out.append((ora.raster_bytes(), ora.macroblocks()))
    return out


_oracle_cache = {}


def oracle_of(builder, w, h, seed=SEED):
    key = (builder, w, h, seed)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle_frames(built(builder, w, h, seed), w, h)
    return _oracle_cache[key]


def resident(ctx, case, seed=SEED):
    builder, w, h = case
    d = aa.Decoder(ctx, w, h)
    for fr in built(builder, w, h, seed).frames:
        d.parse_frame(fr)
    d.upload()
    return d


def check_all(decs, cases, seeds, nframes, what):
    for d, case, seed in zip(decs, cases, seeds):
        want = oracle_of(*case, seed)
        for f in range(min(nframes, len(want))):
            got = d.raster_bytes(f)
            assert got == want[f][0], explain(got, want[f][0], want[f][1], "%s: %s seed %d frame %d" % (what, case_id(case), seed, f))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_hip_matches_oracle_on_directed_motion_streams(gpu_ctx, case):
    builder, w, h = case
    st = built(*case)
    want = oracle_of(*case)
    dec = aa.Decoder(gpu_ctx, w, h)
    for i, fr in enumerate(st.frames):
        shown, fi = dec.get_frame_output(fr)
        assert shown and fi == i
        got = dec.raster_bytes(fi)
        assert got == want[i][0], explain(got, want[i][0], want[i][1], "%s frame %d" % (case_id(case), i))


def test_streams_of_different_sizes_in_one_batch(gpu_ctx):
    """One decode_batch over 16x16, 80x48, 112x80, 144x16 and 33x17 streams (one size twice, with different seeds): the launch's
    max_quads is the batch's, the small frames see quad indices beyond their own count; streams that have run out of frames drop
    out of the later steps."""
    cases = [("edge", 16, 16), ("wave", 80, 48), ("split", 112, 80), ("edge", 144, 16), ("edge", 33, 17), ("wave", 80, 48), ("split", 16, 16)]
    seeds = [SEED, SEED, SEED, SEED, SEED, SEED + 1, SEED]
    decs = [resident(gpu_ctx, c, s) for c, s in zip(cases, seeds)]
    lengths = [len(built(c[0], c[1], c[2], s).frames) for c, s in zip(cases, seeds)]
    for f in range(max(lengths)):
        live = [d for d, n in zip(decs, lengths) if f < n]
        gpu_ctx.decode_batch(live, [f] * len(live))
    check_all(decs, cases, seeds, max(lengths), "mixed batch")


def test_lockstep_copies_and_replay(gpu_ctx):
    """Five copies of the 112x80 wave stream in lock step, all compared; rewind() and replay gives the same bytes (bench.py relies
    on replay being idempotent)."""
    case = ("wave", 112, 80)
    decs = [resident(gpu_ctx, case) for _ in range(5)]
    n = len(built(*case).frames)
    for rep in range(2):
        for f in range(n):
            gpu_ctx.decode_batch(decs, [f] * len(decs))
        check_all(decs, [case] * 5, [SEED] * 5, n, "lock step, pass %d" % rep)
        for d in decs:
            d.rewind()


def test_wave_and_split_streams_under_the_diagonal_schedule(gpu_ctx):
    cases = [c for c in CASES if c[0] in ("wave", "split")]
    try:
        gpu_ctx.set_schedule("diagonal")
        decs = [resident(gpu_ctx, c) for c in cases]
        lengths = [len(built(*c).frames) for c in cases]
        for f in range(max(lengths)):
            live = [d for d, n in zip(decs, lengths) if f < n]
            gpu_ctx.decode_batch(live, [f] * len(live))
        gpu_ctx.sync()
        check_all(decs, cases, [SEED] * len(cases), max(lengths), "diagonal schedule")
    finally:
        gpu_ctx.set_schedule("rows")

