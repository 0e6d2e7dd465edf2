"""What k_reencode_inter asks of a compute unit, read from the code object: alfalfa_amd/csrc/reencode_kernels.hip cross-compiled for gfx950
with the flags alfalfa_amd/build.py uses (device side only, to assembly), and the kernel metadata the compiler writes behind the code.
Nothing else of the assembly is looked at.

The kernel keeps its 4x4 blocks, the census and the candidate costs in registers and must use no private memory (named values and
constant indices are what keeps a lane's arrays out of it: reencode_search.hh says where); its LDS is sixteen slots' pictures of a
macroblock's neighbourhood -- the numbers DESIGN.md 4.12 states.  CPU only; needs hipcc."""
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
    out = str(tmp_path_factory.mktemp("reencode_kernels") / "reencode_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "reencode_kernels.hip"), "-o", out], check=True)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            short = re.search(r"k_reencode_[a-z]+", name.group(1)).group(0)
            kernels[short] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


def test_the_kernel_is_there_and_uses_no_private_memory(metadata):
    assert sorted(metadata) == ["k_reencode_inter"]
    k = metadata["k_reencode_inter"]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k


def test_lds_per_workgroup_is_what_the_design_states(metadata):
    k = metadata["k_reencode_inter"]
    # per slot: the rebase's picture of an intra macroblock's neighbourhood (704 bytes) + bm[16] + the trial's mask, rounded up to 16
    assert k["group_segment_fixed_size"] == 16 * (704 + 16 + 16) == 11776, k
    # one workgroup of four waves per job: a wave may take every register a SIMD lane has for it
    assert k["vgpr_count"] + k.get("agpr_count", 0) <= 512, k
