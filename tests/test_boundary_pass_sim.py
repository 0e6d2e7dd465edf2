"""The two-trip macroblock-boundary pass of a token lane (alfalfa_amd/csrc/tok_fsm.hh) on the host twins: the paths that LEAVE
its common path, each against the host parser record by record and block by block, in both coefficient formats, one lane at a
time (tests/cpp/fsm_sim.cc) and as a wave (tests/cpp/wave_sim.cc).

The common path -- a coded macroblock behind a coded macroblock of the same row -- finds the next macroblock's flags byte, the
above flags of its column and, where the column starts one, the next byte of the Y2 bit array in registers (asked for when the
macroblock before it ended), keeps the current Y2 byte in a register and stores it without reading it first.  What falls back
to reading inside the pass: the first macroblock of a row, a macroblock behind a skipped one, a macroblock the flag ring did
not hold yet when the one before it ended.  What must survive being run twice: a pass that finds the coefficient pool dry.
CPU only."""
import numpy as np
import pytest

import alfalfa_amd as aa
from alfalfa_amd import capi
from conftest import golden_frames
from test_fsm_sim import FORMATS, Sim, check_stream
from test_wave_sim import run_wave


def host_flags(w, h, frames):
    """-> per frame: the flags byte of every macroblock, [mbh, mbw]"""
    host = aa.Parser(w, h)
    return [host.parse(fr)[1].reshape(-1)["flags"].reshape((h + 15) // 16, (w + 15) // 16).copy() for fr in frames]


def coded_stream(w, h, seed, nframes=3, **kw):
    """every macroblock coded (none skipped), a mix of macroblocks with and without a Y2 block"""
    import vp8_synth
    s = vp8_synth.SynthStream(w, h, seed)
    s.frame(key=True, q_index=24, density=0.5, intra_bpred=0.5, **kw)
    for k in range(nframes - 1):
        s.frame(key=False, q_index=30, density=0.4, intra_bpred=0.5, lf_level=8, log2_parts=k % 3, **kw)
    return s.frames


@FORMATS
@pytest.mark.parametrize("mbw", [1, 2, 7, 9, 13, 17, 23])
def test_widths_that_are_not_a_multiple_of_eight_columns(mbw, packed):
    """The Y2 byte in the register covers 8 columns: with 9, 13, 17, 23 columns it is replaced in mid-row (from the early read) and
    again at the row's end (read in the pass), with 1, 2 and 7 every row starts in the byte the last one ended in.  Width 1: every
    macroblock is the first of its row -- the early reads never apply."""
    w, h = 16 * mbw - 5, 80
    frames = coded_stream(w, h, 1000 + mbw)
    fl = host_flags(w, h, frames)
    assert all((f & capi.AA_MB_HAS_Y2).any() and not (f & capi.AA_MB_HAS_Y2).all() for f in fl[:1])     # both kinds: the Y2 bits differ along a row
    check_stream(w, h, frames, packed=packed)


@FORMATS
def test_the_y2_bits_of_a_wide_row_survive_the_register(packed):
    """1080p width (120 columns, 15 Y2 bytes): the contexts of every Y2 block depend on the bit its column's macroblock of the row
    above left -- one wrong or stale byte changes the records of the row below"""
    w, h = 1920, 64
    frames = coded_stream(w, h, 77, nframes=2)
    check_stream(w, h, frames, packed=packed)


@FORMATS
def test_runs_of_skipped_macroblocks_longer_than_the_flag_ring(packed):
    """Skipped macroblocks take no steps, so a run of them gets ahead of the 32-entry flag ring: the coded macroblock behind it was not
    in the ring when the one before ended (nothing was read early: the pass reads for itself), and a coded macroblock right behind a
    skipped one never has early values.  Rows of 120 and 256 columns, nearly everything skipped; the runs are measured from the host
    parser's flags."""
    import vp8_synth
    for w, h, seed, density, runs_over in ((1920, 48, 31, 0.004, 32), (4096, 32, 35, 0.002, 32), (1920, 48, 36, 0.02, 4)):      # (the last: short runs, many coded macroblocks behind a skipped one)
        s = vp8_synth.SynthStream(w, h, seed)
        s.frame(key=True, q_index=30, skip_prob=3, density=density, skip_rate=1.0, intra_bpred=0.3)
        for k in range(3):
            s.frame(key=False, q_index=30, skip_prob=2 + k, density=density, skip_rate=1.0, log2_parts=k % 2, lf_level=8, intra_bpred=0.3)
        longest = 0
        for f in host_flags(w, h, s.frames):
            skipped = np.concatenate([[0], (f.reshape(-1) & capi.AA_MB_SKIP) != 0, [0]]).astype(np.int8)
            edges = np.flatnonzero(np.diff(skipped))
            if len(edges):
                longest = max(longest, int((edges[1::2] - edges[0::2]).max()))
        assert longest > runs_over, longest
        check_stream(w, h, s.frames, packed=packed)


@FORMATS
def test_macroblocks_with_and_without_a_y2_block_alternate(packed):
    """A change of kind at the boundary replaces the slice's Y probability plane (the pass's slow path) and picks the other of the
    two first-block constants; the Y2 bit of a column passes over macroblocks without a Y2 block untouched."""
    import vp8_synth
    w, h = 200, 96
    s = vp8_synth.SynthStream(w, h, 4242)
    s.frame(key=True, q_index=20, density=0.5, intra_bpred=0.5)
    s.frame(key=False, q_index=28, density=0.5, intra_bpred=0.5, prob_inter=120, lf_level=6)
    s.frame(key=False, q_index=28, density=0.3, intra_bpred=0.5, prob_inter=120, skip_prob=128, skip_rate=0.5)
    changes = 0
    for f in host_flags(w, h, s.frames):
        y2 = (f & capi.AA_MB_HAS_Y2) != 0
        changes += int((y2[:, 1:] != y2[:, :-1]).sum())
    assert changes > 50, changes
    check_stream(w, h, s.frames, packed=packed)
    run_wave(w, h, [s.frames] * 3, 5, packed=packed, seed=12)


@FORMATS
def test_the_pool_runs_dry_at_a_boundary(packed):
    """A lane that finds no chunk at a boundary leaves the pass and runs it again later for the same macroblock -- with the early
    values of that macroblock still in its registers: the second pass must find what the first did.  One lane: the frame is handed
    back (TOK_NO_MEMORY, 202) when nothing ever comes, and parses to the host parser's records with exactly the chunks it needs.
    A wave: lanes wait beside decoding wave-mates, take what finished frames give back, and every record is the host parser's."""
    w, h, frames = golden_frames("cif_q60_lf40s5")
    host, sim = aa.Parser(w, h), Sim(w, h, packed)
    hh, hmb, hcf = host.parse(frames[0])
    sim.frame(frames[0])
    took = sim.L.fsm_sim_last_chunks(sim.h)
    if took > 1:
        dry = Sim(w, h, packed)
        dry.L.fsm_sim_set_pool_chunks(dry.h, took - 1)
        dry.frame(frames[0], expect=202)
    exact = Sim(w, h, packed)
    exact.L.fsm_sim_set_pool_chunks(exact.h, took)
    h3, mb3, cf3, _ = exact.frame(frames[0])
    assert h3 == hh and (cf3 == hcf.reshape(-1)).all()
    assert (mb3.view(np.uint8).reshape(-1, 80) == hmb.reshape(-1).view(np.uint8).reshape(-1, 80)).all()
    streams = [coded_stream(320, 176, 800 + k, nframes=4) for k in range(8)]
    plenty = run_wave(320, 176, streams, 16, packed=packed, seed=9)
    need = max(2, plenty["peak_chunks_out"] // 16 + 1)
    scarce = run_wave(320, 176, streams, 16, pool_chunks=need + 1, packed=packed, seed=9)
    assert scarce["periods"] > plenty["periods"]            # lanes stood at boundaries for lack of memory ...
    assert scarce["handed_back"] > 0                        # ... and some handed their frame back and ran it again


@FORMATS
@pytest.mark.parametrize("log2_parts", [0, 1, 2, 3])
def test_partitions_on_one_lane_and_on_a_lane_each(log2_parts, packed):
    """1 / 2 / 4 / 8 DCT partitions: on one lane a row's end is a partition switch (the pass after it starts the row by reading for
    itself); with a lane per partition (the path that keeps the shared uint16 flags and reads them in the pass) the same records."""
    w, h = 16 * 11 - 3, 16 * 9
    frames = coded_stream(w, h, 300 + log2_parts, nframes=3)
    import vp8_synth
    s = vp8_synth.SynthStream(w, h, 310 + log2_parts)
    s.frame(key=True, q_index=20, density=0.4, intra_bpred=0.5, log2_parts=log2_parts, skip_prob=150, skip_rate=0.4)
    s.frame(key=False, q_index=30, density=0.3, intra_bpred=0.5, log2_parts=log2_parts, skip_prob=120, skip_rate=0.5, lf_level=8)
    check_stream(w, h, s.frames, packed=packed)
    run_wave(w, h, [s.frames, frames], 12, packed=packed, seed=3, mp=False)
    run_wave(w, h, [s.frames, frames], 12, packed=packed, seed=3, mp=True)
