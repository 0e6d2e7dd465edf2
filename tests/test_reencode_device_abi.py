"""The device-resident re-encode's entry point without a GPU: aa_reencode_device_batch is exported and bound, refuses null arguments
with its own name in the message, the ABI version stays what it was (a symbol and a struct were added, nothing existing changed), and
the bindings' aa_reencode_device_job has the size and the field offsets a C compiler gives the header's."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from alfalfa_amd import capi
from conftest import ROOT

HEADER_DIR = os.path.join(ROOT, "include")


def test_the_entry_point_is_exported_and_the_version_is_unchanged():
    L = capi.lib()
    assert hasattr(L, "aa_reencode_device_batch") and "aa_reencode_device_batch" in {n for n, _, _ in capi.SYMBOLS}
    assert "aa_reencode_device_batch(" in open(os.path.join(HEADER_DIR, "alfalfa_amd.h")).read()
    assert L.aa_abi_version() == 4


def test_null_arguments_are_refused_without_a_device():
    L = capi.lib()
    assert L.aa_reencode_device_batch(None, None, 0) == -7
    assert b"aa_reencode_device_batch" in L.aa_last_error()
    assert L.aa_reencode_device_batch(None, None, 1) == -7
    assert b"aa_reencode_device_batch" in L.aa_last_error()


def test_there_is_no_append_field():
    assert [n for n, _ in capi.ReencodeDeviceJob._fields_] == ["stream", "hdr", "target", "quality", "num_coeff_blocks", "num_intra_mbs", "frame_index"]


@pytest.mark.skipif(not shutil.which("gcc"), reason="gcc is not installed")
def test_the_job_struct_is_the_header_s(tmp_path):
    fields = [n for n, _ in capi.ReencodeDeviceJob._fields_]
    src, exe = str(tmp_path / "size.c"), str(tmp_path / "size")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "alfalfa_amd.h"\nint main( void ) { printf( "%zu'
                + " %zu" * len(fields) + '\\n", sizeof( aa_reencode_device_job )' + "".join(", offsetof( aa_reencode_device_job, %s )" % n for n in fields) + " ); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", HEADER_DIR, src, "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(capi.ReencodeDeviceJob)] + [getattr(capi.ReencodeDeviceJob, n).offset for n in fields]
    # stream, hdr (8 + 8) | aa_quality_ref (40) | quality (4) | num_coeff_blocks, num_intra_mbs, frame_index (12)
    assert got[0] == 16 + 40 + 4 + 12 == 72
