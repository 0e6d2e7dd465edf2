"""What the two rebase kernels ask of a compute unit, read from the code object: alfalfa_amd/csrc/rebase_kernels.hip cross-compiled for
gfx950 with the flags alfalfa_amd/build.py uses (device side only, to assembly), and the kernel metadata the compiler writes behind
the code.  Nothing else of the assembly is looked at.

Both kernels keep their 4x4 blocks in registers and must use no private memory (the constant indices of their unrolled loops are what
keeps a lane's arrays out of it); k_rebase_inter's LDS is the 16 luma DCs of its four macroblocks, k_rebase_intra's the neighbour
frame of one macroblock -- the numbers DESIGN.md 4.11 states.  CPU only; needs hipcc."""
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
    out = str(tmp_path_factory.mktemp("rebase_kernels") / "rebase_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "rebase_kernels.hip"), "-o", out], check=True)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            short = re.search(r"k_rebase_[a-z]+", name.group(1)).group(0)
            kernels[short] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


def test_both_kernels_are_there_and_use_no_private_memory(metadata):
    assert sorted(metadata) == ["k_rebase_inter", "k_rebase_intra"]
    for name, k in metadata.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 64 and k.get("agpr_count", 0) == 0, (name, k)


def test_lds_per_workgroup_is_what_the_design_states(metadata):
    assert metadata["k_rebase_inter"]["group_segment_fixed_size"] == 4 * 16 * 2                 # the luma DCs of four macroblocks
    # y[17][24] and c[2][9][12], each rounded up to 16 bytes, + edge[16] + pred[16] + dcs[16] of int16
    assert metadata["k_rebase_intra"]["group_segment_fixed_size"] == 416 + 224 + 16 + 16 + 32 == 704
    for name, k in metadata.items():
        assert k["vgpr_count"] <= 128, (name, k)                                                   # four waves per SIMD
