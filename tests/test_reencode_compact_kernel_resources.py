"""What the two compaction kernels of the device-resident re-encode ask of a compute unit, read from the code object:
alfalfa_amd/csrc/reencode_compact_kernels.hip cross-compiled for gfx950 with the flags alfalfa_amd/build.py uses (device side only, to
assembly), and the kernel metadata the compiler writes behind the code.  Nothing else of the assembly is looked at.

The file holds exactly k_reencode_count and k_reencode_compact; they stay in the class of the rebase's pair
(tests/test_rebase_compact_kernel_resources.py), whose statements they share (compact_device.hh): 256 threads a workgroup, a
macroblock each, everything in registers -- the loop-filter level is computed from a parameter record in HBM, not from a private copy
--; k_reencode_count's LDS is its four wave sums, k_reencode_compact's the run's 256 masks and 256 indices and four wave totals.  CPU
only; needs hipcc."""
import os
import re
import shutil
import subprocess

import pytest

from alfalfa_amd import build as B

HIPCC = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """-> {kernel (by the name in the source): {field: int}}"""
    out = str(tmp_path_factory.mktemp("reencode_compact_kernels") / "reencode_compact_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "reencode_compact_kernels.hip"), "-o", out], check=True)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            short = re.search(r"k_[a-z_]+?(?=E[A-Z])", name.group(1)).group(0)
            kernels[short] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


def test_the_file_is_built_into_the_library():
    assert "reencode_compact_kernels.hip" in B.SOURCES
    for header in ("reencode_compact.hh", "compact_device.hh", "rebase_compact.hh"):
        assert header in B.HEADERS, header


def test_both_kernels_are_there_and_use_no_private_memory(metadata):
    assert sorted(metadata) == ["k_reencode_compact", "k_reencode_count"]
    for name, k in metadata.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256 and k.get("agpr_count", 0) == 0, (name, k)


def test_lds_and_registers_stay_in_the_class_of_the_rebase_s_pair(metadata):
    assert metadata["k_reencode_count"]["group_segment_fixed_size"] == 4 * 4                          # the four waves' sums
    assert metadata["k_reencode_compact"]["group_segment_fixed_size"] == 2 * 256 * 4 + 4 * 4 == 2064   # the run's masks and indices, the waves' totals
    for name, k in metadata.items():
        assert k["vgpr_count"] <= 64, (name, k)                                                        # eight waves per SIMD: two workgroups
