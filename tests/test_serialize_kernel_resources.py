"""What k_serialize_tokens, k_token_counts and k_token_probs ask of a compute unit, read from the code object: alfalfa_amd/csrc/serialize_kernels.hip cross-compiled for gfx950
with the flags alfalfa_amd/build.py uses (device side only, to assembly), and the kernel metadata the compiler writes behind the code.
Nothing else of the assembly is looked at.

A lane keeps the boolean encoder, the block walk and the macroblock's context bits in registers: no private memory, no spills
(serialize_common.hh indexes nothing with a run-time value and has one call site per function); and nothing is shared between lanes: no
LDS.  k_token_counts holds one table of branch counts per workgroup in LDS: 2120 words.  The numbers DESIGN.md 4.13 states.  CPU only; needs hipcc."""
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
    out = str(tmp_path_factory.mktemp("serialize_kernels") / "serialize_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "serialize_kernels.hip"), "-o", out], check=True)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            short = re.search(r"k_(serialize|token)_[a-z]+", name.group(1)).group(0)
            kernels[short] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


def test_the_kernel_is_there_and_uses_no_private_memory(metadata):
    assert sorted(metadata) == ["k_serialize_tokens", "k_token_counts", "k_token_probs"]
    for name, threads in (("k_serialize_tokens", 64), ("k_token_counts", 256), ("k_token_probs", 256)):
        k = metadata[name]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == threads, (name, k)


def test_no_lds_and_registers_for_eight_waves_a_simd(metadata):
    k = metadata["k_serialize_tokens"]
    assert k["group_segment_fixed_size"] == 0 and metadata["k_token_probs"]["group_segment_fixed_size"] == 0, k
    assert metadata["k_token_counts"]["group_segment_fixed_size"] == 2120 * 4
    # 512 registers a SIMD lane: the design states 72 for the token lanes (seven waves a SIMD); a few more are tolerated, 128 (four waves) is the bound
    assert k["vgpr_count"] + k.get("agpr_count", 0) <= 128, k
    assert metadata["k_token_counts"]["vgpr_count"] <= 64, metadata["k_token_counts"]
