"""The device compaction of a re-encoded frame's records on the host (tests/cpp/reencode_compact_check.cc: reencode_compact.hh,
rebase_compact.hh and the statements of k_reencode_count / k_reencode_compact, one thread at a time -- count per run of 256 macroblocks,
intra-row words, sum, scan, loop-filter level, scatter -- and what aa_reencode_device_batch derives from the words) against a plain
transcription, written here and not imported from the product, of reencode_records (alfalfa_amd/csrc/runtime_reencode.inc: rebase_records
plus mb_lf_level) and of the row, diagonal and intra-count loops of aa_rebase_device_batch (runtime_rebase.inc), on generated records
and masks.  CPU only; the GPU run of the kernels themselves is tests/test_gpu_reencode_device.py.  The same program, stand-alone and
under AddressSanitizer / UBSan, runs over the same cases."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from alfalfa_amd import capi
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "reencode_compact_check.cc")
CSRC = os.path.join(ROOT, "alfalfa_amd", "csrc")
DEPS = [SRC, os.path.join(ROOT, "include", "alfalfa_amd.h")] + [os.path.join(CSRC, f) for f in ("reencode_compact.hh", "rebase_compact.hh", "parse_common.hh", "vp8_tables.h", "vp8_math.hh")]
FLAGS = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
B_PRED, ZEROMV, SPLITMV = 4, 7, 9
INTER, HAS_Y2, HAS_NONZERO, SKIP, LF_SKIP_INNER = 4, 2, 1, 8, 16
EMITTED = list(range(9))        # every y_mode the re-encode can emit: DC, V, H, TM, B_PRED, NEARESTMV, NEARMV, ZEROMV, NEWMV (never SPLITMV)

# (the header's level, adjustments on, by reference frame, by mode {B_PRED, ZEROMV, the other inter modes, SPLITMV})
LF_OFF = (20, 0, (9, -9, 5, 5), (7, -7, 3, 3))          # adjustments off: the values are there and must not be used
LF_ON = (30, 1, (2, -3, 0, 0), (4, -5, 6, 0))
LF_CLAMP_0 = (5, 1, (-6, -3, 0, 0), (-60, -4, 1, 0))    # intra 0 (B_PRED far below), ZEROMV 0, the other inter modes 3
LF_CLAMP_63 = (60, 1, (2, 1, 0, 0), (40, 3, 2, 0))      # intra 62 (B_PRED 63, from 102), ZEROMV 63 (from 64), the others 63
LF_LEVEL_0 = (0, 1, (10, 10, 10, 10), (10, 10, 10, 10))  # level 0: no filtering whatever the adjustments say


def built(name, extra):
    out = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (out, os.getpid())             # (pytest-xdist workers may build at the same time: rename is atomic)
        subprocess.run(FLAGS + extra + [SRC, "-o", tmp], check=True)
        os.replace(tmp, out)
    return out


def lf_level(lf, ref_frame, y_mode):
    """mb_lf_level (parse_common.hh) for segment 0, statement by statement."""
    level, on, by_ref, by_mode = lf
    if not level:
        return 0
    if on:
        level += by_ref[ref_frame]
        if ref_frame == 0:
            level += by_mode[0] if y_mode == B_PRED else 0
        elif y_mode == ZEROMV:
            level += by_mode[1]
        elif y_mode == SPLITMV:
            level += by_mode[3]
        else:
            level += by_mode[2]
    return 0 if level <= 0 else min(level, 63)


def transcription(rec, masks, dense, mbw, mbh, lf):
    """reencode_records, then the loops aa_rebase_device_batch runs over a frame's records -> (records out, coefficient blocks [n, 16],
    intra-row words, intra macroblocks, diagonals)."""
    out = rec.copy()
    blocks = []
    for i in range(len(rec)):
        inter = rec["ref_frame"][i] != 0
        has_y2 = rec["y_mode"][i] != B_PRED and rec["y_mode"][i] != SPLITMV
        mask = int(masks[i]) & (0x1FFFFFF if has_y2 else 0xFFFFFF)
        out["reserved"][i] = 0
        out["flags"][i] = (INTER if inter else 0) | (HAS_Y2 if has_y2 else 0) | (HAS_NONZERO if mask else SKIP | (LF_SKIP_INNER if has_y2 else 0))
        out["nz_mask"][i] = mask
        out["coeff_index"][i] = len(blocks)
        if mask >> 24:
            blocks.append(dense[i, 24])
        for b in range(24):
            if (mask >> b) & 1:
                blocks.append(dense[i, b])
        out["lf_level"][i] = lf_level(lf, int(out["ref_frame"][i]), int(out["y_mode"][i]))
    words_per_row = (mbw + 63) // 64
    rows = [0] * (words_per_row * mbh)
    diagonals = np.zeros(mbw + 2 * (mbh - 1), np.uint8)
    intra = 0
    for r in range(mbh):
        for col in range(mbw):
            if rec["ref_frame"][r * mbw + col] == 0:
                intra += 1
                diagonals[col + 2 * r] = 1
                rows[r * words_per_row + (col >> 6)] |= 1 << (col & 63)
    return out, np.array(blocks, np.int16).reshape(-1, 16), np.array(rows, np.uint64), intra, diagonals


def generated(mbw, mbh, seed, density=0.5, modes=None, raw_masks=None):
    """mbw * mbh records as the decision leaves them -- every byte it may set (and the compaction must carry over or reset) set to
    something, segment_id 0 --, raw masks and dense slots."""
    nmb = mbw * mbh
    rng = np.random.default_rng(seed)
    rec = np.frombuffer(rng.integers(0, 256, nmb * capi.MB_INFO_DTYPE.itemsize, dtype=np.uint8).tobytes(), capi.MB_INFO_DTYPE).copy()
    rec["y_mode"] = rng.choice(EMITTED, nmb) if modes is None else np.resize(modes, nmb)
    rec["ref_frame"] = np.where(rec["y_mode"] <= 4, 0, 1)            # (every inter candidate predicts from LAST)
    rec["segment_id"] = 0
    if raw_masks is None:
        bits = rng.random((nmb, 25)) < density
        raw_masks = (bits * (1 << np.arange(25))).sum(1) | (rng.integers(0, 2, nmb) << 27)       # (and a bit beyond the 25 slots: never stored)
    dense = rng.integers(-2048, 2048, (nmb, 25, 16)).astype(np.int16)
    return rec, np.asarray(raw_masks, np.uint32), dense, mbw, mbh


def cases():
    """name -> (records, masks, dense, mbw, mbh, filter parameters): 1, 255, 256, 257 and 518 macroblocks; 1, 37, 64, 65 and 130 columns"""
    out = {}
    shapes = [(1, 1, LF_ON), (1, 255, LF_OFF), (255, 1, LF_ON), (64, 4, LF_CLAMP_0), (1, 257, LF_CLAMP_63), (257, 1, LF_LEVEL_0), (37, 14, LF_ON),
              (37, 7, LF_CLAMP_63), (65, 4, LF_CLAMP_0), (130, 2, LF_OFF), (130, 4, LF_CLAMP_63), (64, 8, LF_LEVEL_0)]
    for k, (mbw, mbh, lf) in enumerate(shapes):
        out["random_%dx%d" % (mbw, mbh)] = generated(mbw, mbh, 100 + k) + (lf,)
    # every emitted mode under every filter setting, on the frame whose rows of 37 straddle both run boundaries
    for name, lf in (("off", LF_OFF), ("on", LF_ON), ("clamp_0", LF_CLAMP_0), ("clamp_63", LF_CLAMP_63), ("level_0", LF_LEVEL_0)):
        out["every_mode_37x14_lf_%s" % name] = generated(37, 14, 7, modes=EMITTED) + (lf,)
    out["all_intra_130x4"] = generated(130, 4, 8, modes=[0, 1, 2, 3, B_PRED]) + (LF_ON,)
    out["all_inter_65x4"] = generated(65, 4, 9, modes=[5, 6, 7, 8]) + (LF_ON,)
    out["all_empty_37x14"] = generated(37, 14, 10, raw_masks=np.zeros(518, np.uint32)) + (LF_ON,)
    out["all_25_bits_37x14"] = generated(37, 14, 11, raw_masks=np.full(518, 0x1FFFFFF, np.uint32)) + (LF_CLAMP_63,)
    out["one_intra_last_130x2"] = generated(130, 2, 12, modes=[5] * 259 + [B_PRED]) + (LF_CLAMP_0,)
    return out


CASES = cases()


@pytest.fixture(scope="module")
def expected():
    return {name: transcription(*c) for name, c in CASES.items()}


def test_the_cases_are_what_they_claim(expected):
    assert sorted({c[3] * c[4] for c in CASES.values()} & {1, 255, 256, 257, 518}) == [1, 255, 256, 257, 518]
    assert {1, 37, 64, 65, 130} <= {c[3] for c in CASES.values()}
    for name in ("off", "on", "clamp_0", "clamp_63", "level_0"):
        assert set(CASES["every_mode_37x14_lf_%s" % name][0]["y_mode"].tolist()) == set(EMITTED)
    levels = lambda n: set(expected["every_mode_37x14_lf_%s" % n][0]["lf_level"].tolist())
    assert levels("off") == {20} and levels("level_0") == {0}
    assert levels("on") == {30 + 2, 30 + 2 + 4, 30 - 3 - 5, 30 - 3 + 6}
    assert levels("clamp_0") == {0, 3} and levels("clamp_63") == {62, 63}
    rec, blocks, rows, intra, diagonals = expected["all_intra_130x4"]
    assert intra == 520 and len(rows) == 12 and (rows.reshape(4, 3) == [2**64 - 1, 2**64 - 1, 3]).all() and diagonals.all()
    assert expected["all_inter_65x4"][3] == 0 and not expected["all_inter_65x4"][2].any() and not expected["all_inter_65x4"][4].any()
    rec, blocks, rows, intra, diagonals = expected["one_intra_last_130x2"]
    assert intra == 1 and rows.tolist() == [0, 0, 0, 0, 0, 2] and np.nonzero(diagonals)[0].tolist() == [129 + 2]
    assert len(expected["all_empty_37x14"][1]) == 0 and (expected["all_empty_37x14"][0]["flags"] & SKIP).all()
    rec = expected["all_25_bits_37x14"][0]
    assert len(expected["all_25_bits_37x14"][1]) == int(np.where(rec["y_mode"] == B_PRED, 24, 25).sum())


def lf_bytes(lf):
    return np.array([lf[0], lf[1]] + list(lf[2]) + list(lf[3]) + [0, 0], np.int8)


@pytest.mark.parametrize("name", sorted(CASES))
def test_count_rows_scan_level_scatter_equal_reencode_records(name, expected):
    L = C.CDLL(built("libreencode_compact_check.so", ["-O2", "-fPIC", "-shared"]))
    L.reencode_compact_run.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 2 + [C.c_void_p] * 3 + [C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
    rec, masks, dense, mbw, mbh, lf = CASES[name]
    want_rec, want_blocks, want_rows, want_intra, want_diagonals = expected[name]
    out = np.zeros(len(rec), capi.MB_INFO_DTYPE)
    blocks = np.full((len(want_blocks) + 1, 16), 0x5555, np.int16)         # (one block of room beyond the frame's: it must stay as it is)
    rows = np.full(len(want_rows) + 1, 0x5555, np.uint64)                  # (and one word)
    diagonals = np.full(len(want_diagonals) + 1, 0x55, np.uint8)
    n, intra, params = C.c_uint32(), C.c_uint32(), lf_bytes(lf)

    def run(capacity):
        return L.reencode_compact_run(rec.ctypes.data, masks.ctypes.data, dense.ctypes.data, mbw, mbh, params.ctypes.data, out.ctypes.data, blocks.ctypes.data, capacity,
                                      C.byref(n), rows.ctypes.data, C.byref(intra), diagonals.ctypes.data)

    assert run(len(want_blocks)) == 0
    assert n.value == len(want_blocks) and intra.value == want_intra
    assert (rows[:-1] == want_rows).all(), "%s: intra-row word %d differs" % (name, np.nonzero(rows[:-1] != want_rows)[0][0])
    assert rows[-1] == 0x5555 and (diagonals[:-1] == want_diagonals).all() and diagonals[-1] == 0x55
    differ = np.nonzero(np.frombuffer(out.tobytes(), np.uint8).reshape(len(rec), -1) != np.frombuffer(want_rec.tobytes(), np.uint8).reshape(len(rec), -1))
    assert out.tobytes() == want_rec.tobytes(), "%s: records differ first at macroblock %d, byte %d" % (name, differ[0][0], differ[1][0])
    assert (blocks[:-1] == want_blocks).all(), "%s: block %d differs" % (name, np.nonzero((blocks[:-1] != want_blocks).any(1))[0][0])
    assert (blocks[-1] == 0x5555).all()
    # a coefficient array one block short is refused by the count alone
    if len(want_blocks):
        assert run(len(want_blocks) - 1) == 1


def test_the_same_program_under_the_sanitizers(tmp_path, expected):
    """reencode_compact_check.cc with its own main, built with -fsanitize=address,undefined, over every case: clean, and equal to the transcription."""
    exe = built("reencode_compact_check_asan", ["-O1", "-DREENCODE_COMPACT_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    files = []
    for name in sorted(CASES):
        rec, masks, dense, mbw, mbh, lf = CASES[name]
        want_rec, want_blocks, want_rows, want_intra, want_diagonals = expected[name]
        path = str(tmp_path / (name + ".case"))
        with open(path, "wb") as f:
            f.write(struct.pack("<4I", mbw, mbh, len(want_blocks), want_intra) + lf_bytes(lf).tobytes() + rec.tobytes() + masks.tobytes() + dense.tobytes()
                    + want_rec.tobytes() + want_rows.tobytes() + want_diagonals.tobytes() + want_blocks.tobytes())
        files.append(path)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
