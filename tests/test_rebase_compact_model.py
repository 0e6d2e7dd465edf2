"""The device compaction of a rebased frame's records on the host (tests/cpp/rebase_compact_check.cc: rebase_compact.hh and the statements
of k_rebase_count / k_rebase_compact, one thread at a time -- count per run of 256 macroblocks, sum, scan, scatter) against a plain
transcription of rebase_records (alfalfa_amd/csrc/runtime_rebase.inc), written here and not imported from the product, on generated
masks and records.  CPU only; the GPU run of the kernels themselves is tests/test_gpu_rebase_device.py.  The same program, stand-alone
and under AddressSanitizer / UBSan, runs over the same cases."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from alfalfa_amd import capi
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "rebase_compact_check.cc")
DEPS = [SRC, os.path.join(ROOT, "alfalfa_amd", "csrc", "rebase_compact.hh"), os.path.join(ROOT, "alfalfa_amd", "csrc", "vp8_math.hh"),
        os.path.join(ROOT, "include", "alfalfa_amd.h")]
FLAGS = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
B_PRED, SPLITMV = 4, 9
INTER, HAS_Y2, HAS_NONZERO, SKIP, LF_SKIP_INNER = 4, 2, 1, 8, 16


def built(name, extra):
    out = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (out, os.getpid())             # (pytest-xdist workers may build at the same time: rename is atomic)
        subprocess.run(FLAGS + extra + [SRC, "-o", tmp], check=True)
        os.replace(tmp, out)
    return out


def transcription(rec, masks, dense):
    """rebase_records, statement by statement -> (records out, coefficient blocks [n, 16])."""
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
    return out, np.array(blocks, np.int16).reshape(-1, 16)


def generated(nmb, seed, density=0.5, modes=None, raw_masks=None):
    """nmb records with every byte the compaction must carry over (or reset) set to something, raw masks and dense slots."""
    rng = np.random.default_rng(seed)
    rec = np.frombuffer(rng.integers(0, 256, nmb * capi.MB_INFO_DTYPE.itemsize, dtype=np.uint8).tobytes(), capi.MB_INFO_DTYPE).copy()
    rec["y_mode"] = rng.integers(0, 10, nmb) if modes is None else modes
    rec["ref_frame"] = np.where(rec["y_mode"] <= 4, 0, rng.integers(1, 4, nmb))
    if raw_masks is None:
        bits = rng.random((nmb, 25)) < density
        raw_masks = (bits * (1 << np.arange(25))).sum(1) | (rng.integers(0, 2, nmb) << 27)       # (and a bit beyond the 25 slots: never stored)
    dense = rng.integers(-2048, 2048, (nmb, 25, 16)).astype(np.int16)
    return rec, np.asarray(raw_masks, np.uint32), dense


def cases():
    out = {}
    for nmb in (1, 255, 256, 257, 2 * 256 + 1):
        out["random_%d" % nmb] = generated(nmb, nmb)
    out["sparse_513"] = generated(513, 7, density=0.04)
    out["all_empty_257"] = generated(257, 8, raw_masks=np.zeros(257, np.uint32))
    out["all_empty_1"] = generated(1, 9, raw_masks=np.zeros(1, np.uint32))
    out["all_25_bits_513"] = generated(513, 10, modes=np.resize([0, 1, 2, 3, 5, 6, 7, 8], 513), raw_masks=np.full(513, 0x1FFFFFF, np.uint32))
    # B_PRED / SPLITMV macroblocks whose raw mask has bit 24 set: the bit is dropped -- alone (nothing stored: a skipped macroblock) and beside others
    out["no_y2_raw_bit24_300"] = generated(300, 11, modes=np.resize([B_PRED, SPLITMV, 0, 8], 300), raw_masks=np.resize([1 << 24, 0x1FFFFFF, 1 << 24, 0x1000001], 300))
    out["y2_alone_258"] = generated(258, 12, modes=np.resize([0, 5, 3, 8, 7], 258), raw_masks=np.full(258, 1 << 24, np.uint32))
    return out


CASES = cases()


@pytest.fixture(scope="module")
def expected():
    return {name: transcription(*c) for name, c in CASES.items()}


def test_the_cases_are_what_they_claim(expected):
    assert len(expected["all_empty_257"][1]) == 0 and (expected["all_empty_257"][0]["flags"] & SKIP).all()
    assert len(expected["all_25_bits_513"][1]) == 25 * 513
    rec, blocks = expected["no_y2_raw_bit24_300"]
    assert (rec["nz_mask"][0::4] == 0).all() and (rec["nz_mask"][1::4] == 0xFFFFFF).all() and (rec["nz_mask"][2::4] == 1 << 24).all()
    assert (rec["flags"][0] & (SKIP | HAS_Y2 | LF_SKIP_INNER)) == SKIP
    rec, blocks = expected["y2_alone_258"]
    assert len(blocks) == 258 and (rec["nz_mask"] == 1 << 24).all() and (blocks == CASES["y2_alone_258"][2][:, 24]).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_count_scan_scatter_equals_rebase_records(name, expected):
    L = C.CDLL(built("librebase_compact_check.so", ["-O2", "-fPIC", "-shared"]))
    L.rebase_compact_run.argtypes = [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 2 + [C.c_uint32, C.POINTER(C.c_uint32)]
    rec, masks, dense = CASES[name]
    want_rec, want_blocks = expected[name]
    out = np.zeros(len(rec), capi.MB_INFO_DTYPE)
    blocks = np.full((len(want_blocks) + 1, 16), 0x5555, np.int16)         # (one block of room beyond the frame's: it must stay as it is)
    n = C.c_uint32()
    assert L.rebase_compact_run(rec.ctypes.data, masks.ctypes.data, dense.ctypes.data, len(rec), out.ctypes.data, blocks.ctypes.data, len(want_blocks), C.byref(n)) == 0
    assert n.value == len(want_blocks)
    differ = np.nonzero(np.frombuffer(out.tobytes(), np.uint8).reshape(len(rec), -1) != np.frombuffer(want_rec.tobytes(), np.uint8).reshape(len(rec), -1))
    assert out.tobytes() == want_rec.tobytes(), "%s: records differ first at macroblock %d, byte %d" % (name, differ[0][0], differ[1][0])
    assert (blocks[:-1] == want_blocks).all(), "%s: block %d differs" % (name, np.nonzero((blocks[:-1] != want_blocks).any(1))[0][0])
    assert (blocks[-1] == 0x5555).all()
    # a coefficient array one block short is refused by the count alone
    if len(want_blocks):
        assert L.rebase_compact_run(rec.ctypes.data, masks.ctypes.data, dense.ctypes.data, len(rec), out.ctypes.data, blocks.ctypes.data, len(want_blocks) - 1, C.byref(n)) == 1


def test_the_same_program_under_the_sanitizers(tmp_path, expected):
    """rebase_compact_check.cc with its own main, built with -fsanitize=address,undefined, over every case: clean, and equal to the transcription."""
    exe = built("rebase_compact_check_asan", ["-O1", "-DREBASE_COMPACT_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    files = []
    for name in sorted(CASES):
        rec, masks, dense = CASES[name]
        want_rec, want_blocks = expected[name]
        path = str(tmp_path / (name + ".case"))
        with open(path, "wb") as f:
            f.write(struct.pack("<2I", len(rec), len(want_blocks)) + rec.tobytes() + masks.tobytes() + dense.tobytes() + want_rec.tobytes() + want_blocks.tobytes())
        files.append(path)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
