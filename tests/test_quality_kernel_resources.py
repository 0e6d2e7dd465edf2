"""What the two quality kernels ask of a compute unit, read from the code object: alfalfa_amd/csrc/quality_kernels.hip cross-compiled
for gfx950 with the flags alfalfa_amd/build.py uses (device side only, to assembly), and the kernel metadata the compiler writes
behind the code.

k_quality_blocks streams both planes through a CU once: it must use no private memory, and its block sums -- nine block rows of
484 columns, three words each -- must leave room for three workgroups in a CU's 160 KB of LDS.  k_quality_sum is one wave with a
4 KB stage.  The block sums come from v_dot4_u32_u8 on the packed bytes, and the only atomic is the integer one of the squared
error: no float atomics, no compare-and-swap loop.  CPU only; needs hipcc."""
import os
import re
import shutil
import subprocess

import pytest

from alfalfa_amd import build as B

HIPCC = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("quality_kernels") / "quality_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "quality_kernels.hip"), "-o", out], check=True)
    return open(out).read()


@pytest.fixture(scope="module")
def metadata(assembly):
    """-> {kernel (by the name in the source): {field: int}}"""
    meta = assembly[assembly.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name:
            short = re.search(r"k_quality_[a-z]+", name.group(1)).group(0)
            kernels[short] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


def test_both_kernels_are_there_and_use_no_private_memory(metadata):
    assert sorted(metadata) == ["k_quality_blocks", "k_quality_sum"]
    for name, k in metadata.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["wavefront_size"] == 64 and k.get("agpr_count", 0) == 0, (name, k)


def test_three_block_workgroups_fit_a_compute_unit(metadata):
    k = metadata["k_quality_blocks"]
    rows, cols = 8 + 1, 480 + 4                              # AA_QUALITY_STRIP_ROWS + 1, AA_QUALITY_CHUNK_WINDOWS + 4
    assert k["group_segment_fixed_size"] == rows * 3 * cols * 4 + 4 * 8      # block sums + the four waves' squared errors
    assert 3 * k["group_segment_fixed_size"] <= 160 * 1024
    assert k["max_flat_workgroup_size"] == 256
    assert k["vgpr_count"] <= 128                            # 512 / 128 = 4 waves per SIMD: the 12 waves of three workgroups fit
    s = metadata["k_quality_sum"]
    assert s["group_segment_fixed_size"] == 1024 * 4 and s["max_flat_workgroup_size"] == 64


def test_dot4_on_packed_bytes_wide_loads_and_one_integer_atomic(assembly):
    assert assembly.count("v_dot4_u32_u8") >= 80             # 4 blocks x 4 rows x 5 sums per tile
    assert assembly.count("global_load_dwordx4") >= 8        # 4 rows x 2 planes per tile (and the stage of the second pass)
    assert "flat_load" not in assembly
    atomics = re.findall(r"\b(?:global|flat|ds)_atomic_\w+", assembly)
    assert atomics == ["global_atomic_add_x2"], atomics
    assert "cmpswap" not in assembly
