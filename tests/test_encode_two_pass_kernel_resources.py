"""What the second pass's kernels ask of a compute unit, read from the code object: alfalfa_amd/csrc/encode_two_pass_kernels.hip
cross-compiled for gfx950 with the flags alfalfa_amd/build.py uses (device side only, to assembly), and the kernel metadata the compiler
writes behind the code.  Nothing else of the assembly is looked at.

k_encode_key2 is k_encode_key's macroblock code under Key2Policy: the lane's sixteen coefficients and its trellis (2 x 16 node words, two
live rate / distortion pairs) stay in registers -- no private memory, no vector register spilled -- and the LDS is the sixteen pictures
k_encode_key has; the token costs are read from global memory, not staged.  The numbers are pinned at what the build shows.  CPU only;
needs hipcc."""
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
    out = str(tmp_path_factory.mktemp("encode_two_pass_kernels") / "encode_two_pass_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "encode_two_pass_kernels.hip"), "-o", out], check=True)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            short = re.search(r"k_[a-z0-9_]+?(?=EPK|$)", name.group(1)).group(0)
            kernels[short] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


def test_the_three_kernels_and_no_private_memory(metadata):
    assert sorted(metadata) == ["k_encode_key2", "k_key2_first_pass", "k_key2_updates"]
    for name, k in metadata.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_lds_and_registers_are_what_the_build_shows(metadata):
    k = metadata["k_encode_key2"]
    # per slot: the rebase's picture of an intra macroblock's neighbourhood (704 bytes) + bm[16] + the trial's mask, rounded up to 16 --
    # k_encode_key's; the trellis adds nothing to it
    assert k["group_segment_fixed_size"] == 16 * (704 + 16 + 16) == 11776, k
    # one workgroup of four waves per job: a wave may take every register a SIMD lane has for it (512)
    assert k["vgpr_count"] + k.get("agpr_count", 0) <= 512 and k["vgpr_count"] == KEY2_VGPRS and k.get("agpr_count", 0) == KEY2_AGPRS, k
    assert k["sgpr_count"] <= 106, k
    # the branch counts [4][8][3][11][2] of one workgroup
    assert metadata["k_key2_first_pass"]["group_segment_fixed_size"] == 2112 * 4
    assert metadata["k_key2_updates"]["group_segment_fixed_size"] == 0


KEY2_VGPRS, KEY2_AGPRS = 275, 0
