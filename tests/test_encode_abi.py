"""The forward encoder's part of the C ABI: the symbols include/alfalfa_amd.h declares for it are exported and bound, the prototypes
stand in the header, the job structures are the re-encode's (typedefs), and what the calls refuse without a device.  CPU only."""
import ctypes as C
import os
import re

from alfalfa_amd import capi
from conftest import ROOT
from test_capi import declared_symbols

NEW = ["aa_encode_batch", "aa_encode_device_batch", "aa_encode_last_timing"]


def test_the_new_symbols_are_declared_exported_and_bound():
    L = capi.lib()
    declared, bound = declared_symbols(), {n for n, _, _ in capi.SYMBOLS}
    for n in NEW:
        assert n in declared and hasattr(L, n) and n in bound, n


def test_the_prototypes_and_the_job_types_stand_in_the_header():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "alfalfa_amd.h")).read())
    for line in ("typedef aa_reencode_job aa_encode_job;", "typedef aa_reencode_device_job aa_encode_device_job;",
                 "aa_status aa_encode_batch( aa_ctx * ctx, aa_encode_job * jobs, int n );",
                 "aa_status aa_encode_device_batch( aa_ctx * ctx, aa_encode_device_job * jobs, int n );",
                 "aa_status aa_encode_last_timing( aa_ctx * ctx, double out[5] );"):
        assert line in text, line
    assert capi.EncodeJob is capi.ReencodeJob and capi.EncodeDeviceJob is capi.ReencodeDeviceJob
    assert C.sizeof(capi.EncodeJob) == 96 and C.sizeof(capi.EncodeDeviceJob) == 16 + 40 + 4 + 12
    assert "#define AA_ABI_VERSION 4" in text and capi.lib().aa_abi_version() == 4          # (an addition: the version stands)


def test_refusals_that_need_no_device():
    L = capi.lib()
    jobs = (capi.EncodeJob * 1)()
    djobs = (capi.EncodeDeviceJob * 1)()
    assert L.aa_encode_batch(None, None, 1) == -7 and L.aa_last_error().startswith(b"aa_encode_batch:")
    assert L.aa_encode_batch(None, jobs, 1) == -7 and L.aa_encode_batch(None, jobs, 0) == -7
    assert L.aa_encode_device_batch(None, None, 1) == -7 and L.aa_last_error().startswith(b"aa_encode_device_batch:")
    assert L.aa_encode_device_batch(None, djobs, 0) == -7
    assert L.aa_encode_last_timing(None, None) == -7 and b"aa_encode_last_timing" in L.aa_last_error()
