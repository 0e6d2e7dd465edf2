"""The re-encode's part of the C ABI: the symbols include/alfalfa_amd.h declares for it are exported and bound, and the job structure
has the layout the header gives it (tests/test_capi.py checks every declared symbol; these are the ones this call added).  CPU only."""
import ctypes as C

from alfalfa_amd import capi
from test_capi import declared_symbols

NEW = ["aa_reencode_batch", "aa_reencode_last_timing", "aa_ctx_set_reencode_slots"]


def test_the_new_symbols_are_declared_exported_and_bound():
    L = capi.lib()
    declared, bound = declared_symbols(), {n for n, _, _ in capi.SYMBOLS}
    for n in NEW:
        assert n in declared and hasattr(L, n) and n in bound, n


def test_the_job_structure_is_the_header_s():
    # stream, hdr (8 + 8) | aa_quality_ref (40) | quality, append (4 + 4) | mbs_out, coeffs_out, capacity (24) | num_coeff_blocks, frame_index (4 + 4)
    assert C.sizeof(capi.ReencodeJob) == 16 + 40 + 8 + 24 + 8
    assert capi.ReencodeJob.target.offset == 16 and capi.ReencodeJob.quality.offset == 56 and capi.ReencodeJob.mbs_out.offset == 64
    assert capi.ReencodeJob.frame_index.offset == 92


def test_refusals_that_need_no_device():
    L = capi.lib()
    assert L.aa_reencode_batch(None, None, 1) == -7 and b"aa_reencode_batch" in L.aa_last_error()
    assert L.aa_reencode_last_timing(None, None) == -7
    assert L.aa_ctx_set_reencode_slots(None, 4) == -7
