"""What k_hash_chains asks of a compute unit, read from the code object: alfalfa_amd/csrc/hash_kernels.hip cross-compiled for gfx950
with the flags alfalfa_amd/build.py uses (device side only, to assembly), and the kernel metadata the compiler writes behind the code.

A lane walks a chain of millions of dependent steps with two 16-byte loads in flight: a spill would put a scratch access into every
step, and LDS would serve nothing -- lanes share nothing.  The register count is what profiles/hash_batch.md records.  CPU only;
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
    """-> the metadata fields of k_hash_chains as integers"""
    out = str(tmp_path_factory.mktemp("hash_kernels") / "hash_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "hash_kernels.hip"), "-o", out], check=True)
    assembly = open(out).read()
    meta = assembly[assembly.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name and "k_hash_chains" in name.group(1):
            kernels["k_hash_chains"] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    assert sorted(kernels) == ["k_hash_chains"]
    return kernels["k_hash_chains"]


def test_no_scratch_and_no_lds(metadata):
    k = metadata
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 64 and k.get("agpr_count", 0) == 0, k


def test_vector_registers(metadata):
    print("k_hash_chains: %d VGPRs, %d SGPRs" % (metadata["vgpr_count"], metadata["sgpr_count"]))
    assert metadata["vgpr_count"] <= 64, metadata
