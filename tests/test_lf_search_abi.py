"""The batched loop-filter level search's entry points without a GPU: aa_lf_search_decode_batch, aa_ctx_set_lf_search_round and
aa_lf_search_last_timing are exported and bound, null arguments are refused with the call's own name in the message, the ABI version
stays what it was (symbols and a struct were added, nothing existing changed), and the bindings' aa_lf_search_job has the size and the
field offsets a C compiler gives the header's."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import alfalfa_amd as aa
from alfalfa_amd import capi
from conftest import ROOT

HEADER_DIR = os.path.join(ROOT, "include")
NEW = ["aa_lf_search_decode_batch", "aa_ctx_set_lf_search_round", "aa_lf_search_last_timing"]


def test_the_entry_points_are_exported_and_the_version_is_unchanged():
    L = capi.lib()
    header = open(os.path.join(HEADER_DIR, "alfalfa_amd.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in {n for n, _, _ in capi.SYMBOLS} and name + "(" in header, name
    assert L.aa_abi_version() == 4
    assert (capi.AA_LF_MEASURE_SSIM, capi.AA_LF_MEASURE_SSE) == (0, 1) and "#define AA_LF_MEASURE_SSE 1" in header


def test_null_arguments_are_refused_without_a_device():
    L = capi.lib()
    for n in (0, 1, -1):
        assert L.aa_lf_search_decode_batch(None, None, n, 0) == -7
        assert L.aa_last_error().startswith(b"aa_lf_search_decode_batch:")
    assert L.aa_ctx_set_lf_search_round(None, 4, 0) == -7 and b"aa_ctx_set_lf_search_round" in L.aa_last_error()
    assert L.aa_lf_search_last_timing(None, None) == -7 and b"aa_lf_search_last_timing" in L.aa_last_error()


def test_the_python_surface_is_there():
    for owner, name in ((aa.Context, "lf_search_decode"), (aa.Context, "set_lf_search_round"), (aa.Context, "lf_search_timing"), (aa.Decoder, "lf_search_decode")):
        assert callable(getattr(owner, name))
    ext = {"lf_delta_update": 0, "ref_lf_update": [0, 1, 0, 0], "ref_lf_delta": [0, 3, 0, 0], "mode_lf_update": [0] * 4, "mode_lf_delta": [0] * 4, "skip_enabled": 1}
    out = aa.with_zero_lf_deltas(ext)
    assert out == {"lf_delta_update": 1, "ref_lf_update": [1] * 4, "ref_lf_delta": [0] * 4, "mode_lf_update": [1] * 4, "mode_lf_delta": [0] * 4, "skip_enabled": 1}
    assert ext["lf_delta_update"] == 0 and ext["ref_lf_delta"] == [0, 3, 0, 0], "the helper changed its argument"
    capi.FrameHeaderExt.from_dict(out)


@pytest.mark.skipif(not shutil.which("gcc"), reason="gcc is not installed")
def test_the_job_struct_is_the_header_s(tmp_path):
    fields = [n for n, _ in capi.LfSearchJob._fields_]
    assert fields == ["stream", "frame_index", "original", "level_lo", "level_hi", "best_level", "evaluated", "best_score"]
    src, exe = str(tmp_path / "size.c"), str(tmp_path / "size")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "alfalfa_amd.h"\nint main( void ) { printf( "%zu'
                + " %zu" * len(fields) + '\\n", sizeof( aa_lf_search_job )' + "".join(", offsetof( aa_lf_search_job, %s )" % n for n in fields) + " ); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", HEADER_DIR, src, "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(capi.LfSearchJob)] + [getattr(capi.LfSearchJob, n).offset for n in fields]
    # stream (8) | frame_index (4 + 4 of padding) | aa_quality_ref (40) | level_lo, level_hi, best_level, evaluated (16) | best_score (8)
    assert got[0] == 8 + 8 + 40 + 16 + 8 == 80
