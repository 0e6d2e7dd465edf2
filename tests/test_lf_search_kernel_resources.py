"""What k_lf_candidates, k_lf_choose and k_lf_finish ask of a compute unit, read from the code object: alfalfa_amd/csrc/lf_search_kernels.hip
cross-compiled for gfx950 with the flags alfalfa_amd/build.py uses (device side only, to assembly), and the kernel metadata the compiler
writes behind the code.  Nothing else of the assembly is looked at.

The three kernels are plain grids: a thread keeps the pieces it copies and the state of its search in registers -- no private memory, no
spills -- and nothing is shared between threads: no LDS.  The register counts are stated in DESIGN.md 4.14 and not fixed here.  CPU only;
needs hipcc."""
import os
import re
import shutil
import subprocess

import pytest

from alfalfa_amd import build as B

HIPCC = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc is not installed")
KERNELS = {"k_lf_candidates": 256, "k_lf_choose": 64, "k_lf_finish": 256}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lf_search_kernels") / "lf_search_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "lf_search_kernels.hip"), "-o", out], check=True)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            short = re.search(r"k_lf_[a-z]+", name.group(1)).group(0)
            kernels[short] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


def test_the_source_is_part_of_the_library():
    assert "lf_search_kernels.hip" in B.SOURCES and "lf_choose.hh" in B.HEADERS


def test_the_kernels_are_there_and_use_no_private_memory(metadata):
    assert sorted(metadata) == sorted(KERNELS)
    for name, threads in KERNELS.items():
        k = metadata[name]
        print(name, "vgprs", k["vgpr_count"], "sgprs", k["sgpr_count"])
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == threads, (name, k)


def test_no_lds(metadata):
    for name in KERNELS:
        assert metadata[name]["group_segment_fixed_size"] == 0, (name, metadata[name])
