"""What k_encode_key and k_encode_inter ask of a compute unit, read from the code object: alfalfa_amd/csrc/encode_kernels.hip
cross-compiled for gfx950 with the flags alfalfa_amd/build.py uses (device side only, to assembly), and the kernel metadata the compiler
writes behind the code.  Nothing else of the assembly is looked at.

Both kernels are k_reencode_inter's macroblock code under another policy of the decision: no private memory, no register spilled to
memory, the same sixteen LDS pictures.  The key kernel carries no inter candidate -- it needs a quarter fewer vector registers than the
inter kernel -- and the numbers are pinned at what the build shows.  CPU only; needs hipcc."""
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
    out = str(tmp_path_factory.mktemp("encode_kernels") / "encode_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "encode_kernels.hip"), "-o", out], check=True)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            short = re.search(r"k_[a-z_]+?(?=EPK|$)", name.group(1)).group(0)
            kernels[short] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


def test_exactly_the_two_kernels_and_no_private_memory(metadata):
    assert sorted(metadata) == ["k_encode_inter", "k_encode_key"]
    for name, k in metadata.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_lds_and_registers_are_what_the_build_shows(metadata):
    for name, k in metadata.items():
        # per slot: the rebase's picture of an intra macroblock's neighbourhood (704 bytes) + bm[16] + the trial's mask, rounded up to 16
        assert k["group_segment_fixed_size"] == 16 * (704 + 16 + 16) == 11776, (name, k)
        assert k.get("agpr_count", 0) == 0, (name, k)
    # one workgroup of four waves per job: a wave may take every register a SIMD lane has for it (512)
    assert metadata["k_encode_key"]["vgpr_count"] == KEY_VGPRS, metadata["k_encode_key"]
    assert metadata["k_encode_inter"]["vgpr_count"] == INTER_VGPRS, metadata["k_encode_inter"]
    assert metadata["k_encode_key"]["sgpr_count"] <= 106 and metadata["k_encode_inter"]["sgpr_count"] <= 106
    # scalar registers beyond the file are parked in lanes of vector registers, as k_reencode_inter's are (55 there): none goes to memory
    # (private_segment_fixed_size == 0 above)
    assert metadata["k_encode_key"]["sgpr_spill_count"] == KEY_SGPRS_PARKED and metadata["k_encode_inter"]["sgpr_spill_count"] == INTER_SGPRS_PARKED


KEY_VGPRS, INTER_VGPRS = 195, 258
KEY_SGPRS_PARKED, INTER_SGPRS_PARKED = 47, 54
