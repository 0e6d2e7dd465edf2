"""The size estimate's and the target-size search's entry points without a GPU: the five symbols are declared, exported and bound, null
arguments are refused with the call's own name in front, the ABI version stays what it was (symbols and two structs were added, nothing
existing changed), the bindings' job structs have the sizes and field offsets a C compiler gives the header's, and the starting range
is the reference's (encoder.cc:597-608)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import alfalfa_amd as aa
from alfalfa_amd import capi
from conftest import ROOT
from test_capi import declared_symbols

HEADER_DIR = os.path.join(ROOT, "include")
NEW = ["aa_estimate_size_batch", "aa_target_size_batch", "aa_target_size_range", "aa_ctx_set_target_size_round", "aa_target_size_last_timing"]


def test_the_entry_points_are_declared_exported_and_bound_and_the_version_is_unchanged():
    L = capi.lib()
    declared, bound = declared_symbols(), {n for n, _, _ in capi.SYMBOLS}
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in bound, name
    header = open(os.path.join(HEADER_DIR, "alfalfa_amd.h")).read()
    assert "#define AA_ABI_VERSION 4" in header and L.aa_abi_version() == 4


def test_null_arguments_are_refused_without_a_device():
    L = capi.lib()
    ej, tj = (capi.EstimateSizeJob * 1)(), (capi.TargetSizeJob * 1)()
    for call, jobs, name in ((L.aa_estimate_size_batch, ej, b"aa_estimate_size_batch:"), (L.aa_target_size_batch, tj, b"aa_target_size_batch:")):
        for args in ((None, None, 1), (None, jobs, 1), (None, jobs, 0), (None, jobs, -1)):
            assert call(*args) == -7 and L.aa_last_error().startswith(name), (name, args)
    assert ej[0].size_out == 0 and tj[0].estimates == 0 and tj[0].q_index == 0, "a refused call wrote an output field"
    assert L.aa_ctx_set_target_size_round(None, 0) == -7 and b"aa_ctx_set_target_size_round" in L.aa_last_error()
    assert L.aa_target_size_last_timing(None, None) == -7 and b"aa_target_size_last_timing" in L.aa_last_error()


def test_the_python_surface_is_there():
    for owner, name in ((aa.Context, "estimate_frame_sizes"), (aa.Context, "target_size_q"), (aa.Context, "set_target_size_round"), (aa.Context, "target_size_timing"),
                        (aa.Decoder, "estimate_frame_size"), (aa.Decoder, "target_size_q")):
        assert callable(getattr(owner, name))
    assert aa.estimate_carry() == (0, 0, 0, 0)


def test_the_starting_range_is_the_reference_s():
    assert aa.target_size_range() == (4, 127) and aa.target_size_range(None) == (4, 127)
    for last in range(128):
        lo, hi = 4, 127                      # encoder.cc:597-608, restated
        if last - 16 >= lo:
            lo = last - 16
        hi = min(hi, last + 16)
        assert aa.target_size_range(last) == (lo, hi), last
    assert aa.target_size_range(127) == (111, 127) and aa.target_size_range(19) == (4, 35) and aa.target_size_range(20) == (4, 36) and aa.target_size_range(0) == (4, 16)


@pytest.mark.skipif(not shutil.which("gcc"), reason="gcc is not installed")
@pytest.mark.parametrize("ctype, name", [(capi.EstimateSizeJob, "aa_estimate_size_job"), (capi.TargetSizeJob, "aa_target_size_job")])
def test_the_job_structs_are_the_header_s(tmp_path, ctype, name):
    fields = [n for n, _ in ctype._fields_]
    src, exe = str(tmp_path / "size.c"), str(tmp_path / "size")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "alfalfa_amd.h"\nint main( void ) { printf( "%zu'
                + " %zu" * len(fields) + '\\n", sizeof( ' + name + " )" + "".join(", offsetof( %s, %s )" % (name, n) for n in fields) + " ); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", HEADER_DIR, src, "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(ctype)] + [getattr(ctype, n).offset for n in fields]
    # stream (8) | aa_quality_ref (40) | key_frame, quality, q_index (12) | carry (4) | size_out (8)
    # stream (8) | aa_quality_ref (40) | key_frame, quality, q_lo, q_hi (16) | target_size (8) | carry (4) | q_index, estimates (8) | visited_q (32 + 4 of padding) | visited_size (64)
    assert got[0] == {"aa_estimate_size_job": 72, "aa_target_size_job": 184}[name]
