"""What k_estimate_key, k_estimate_inter and k_estimate_tokens ask of a compute unit, read from the code object:
alfalfa_amd/csrc/estimate_kernels.hip cross-compiled for gfx950 with the flags alfalfa_amd/build.py uses (device side only, to assembly),
and the kernel metadata the compiler writes behind the code.  Nothing else of the assembly is looked at.

The two decision kernels are k_encode_key's and k_encode_inter's macroblock code under the sampled policies: no private memory, no
vector register spilled, the same sixteen LDS pictures and no more -- the LDS is k_encode_inter's, compiled here beside them.  The
token kernel is a lane per job that keeps its boolean encoder in registers and stores nothing but its three words: no LDS, no
private memory.  CPU only; needs hipcc."""
import os
import re
import shutil
import subprocess

import pytest

from alfalfa_amd import build as B

HIPCC = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc is not installed")


def kernels_of(source, out):
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, source), "-o", out], check=True)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            short = re.search(r"k_[a-z_]+?(?=EPK|$)", name.group(1)).group(0)
            kernels[short] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    d = tmp_path_factory.mktemp("estimate_kernels")
    return kernels_of("estimate_kernels.hip", str(d / "estimate_kernels.s")), kernels_of("encode_kernels.hip", str(d / "encode_kernels.s"))


def test_exactly_the_three_kernels_no_private_memory_no_vector_spill(metadata):
    est, _ = metadata
    assert sorted(est) == ["k_estimate_inter", "k_estimate_key", "k_estimate_tokens"]
    for name, k in est.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["wavefront_size"] == 64 and k.get("agpr_count", 0) == 0, (name, k)
    assert est["k_estimate_key"]["max_flat_workgroup_size"] == est["k_estimate_inter"]["max_flat_workgroup_size"] == 256
    assert est["k_estimate_tokens"]["max_flat_workgroup_size"] == 64


def test_lds_is_no_more_than_the_forward_inter_kernel_s(metadata):
    est, enc = metadata
    limit = enc["k_encode_inter"]["group_segment_fixed_size"]
    assert limit == 16 * (704 + 16 + 16)
    assert est["k_estimate_key"]["group_segment_fixed_size"] <= limit and est["k_estimate_inter"]["group_segment_fixed_size"] <= limit
    assert est["k_estimate_tokens"]["group_segment_fixed_size"] == 0
    # the registers are pinned at what the build shows, as the forward kernels' are (195 / 258 there: the sampled key kernel needs fewer,
    # the inter kernel as many); the scalar registers beyond the file are parked in lanes of vector registers, none goes to memory
    # (private_segment_fixed_size == 0 above)
    assert est["k_estimate_key"]["vgpr_count"] == KEY_VGPRS and est["k_estimate_inter"]["vgpr_count"] == INTER_VGPRS, (est["k_estimate_key"], est["k_estimate_inter"])
    assert est["k_estimate_key"]["sgpr_spill_count"] == KEY_SGPRS_PARKED and est["k_estimate_inter"]["sgpr_spill_count"] == INTER_SGPRS_PARKED
    # the token lane: a boolean encoder, the neighbours' masks, the columns' Y2 bits and a block's coefficients' addresses
    assert est["k_estimate_tokens"]["vgpr_count"] == TOKEN_VGPRS and est["k_estimate_tokens"]["sgpr_spill_count"] == 0, est["k_estimate_tokens"]


KEY_VGPRS, INTER_VGPRS, TOKEN_VGPRS = 166, 256, 79
KEY_SGPRS_PARKED, INTER_SGPRS_PARKED = 49, 53
