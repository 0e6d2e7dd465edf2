"""What the token worker kernel asks of a compute unit, read from the code object: alfalfa_amd/csrc/parse_kernels.hip cross-compiled
for gfx950 with the flags alfalfa_amd/build.py uses (device side only, to assembly), and the kernel metadata the compiler writes
behind the code.

k_token_workers<true, false> -- packed coefficients, a lane of its own per frame -- is the instantiation the benchmark runs, and
it is resident: what it holds of a CU is what the reconstruction kernels do not get.  It must use no private memory (scratch
traffic shares the vector-memory queue with the coefficient store of every step), no static LDS (its dynamic request is exactly
what 30 lanes need, so that three workgroups leave a CU room for three loop-filter workgroups) and few enough registers for a
256-register loop-filter wave to share its SIMD.  CPU only; needs hipcc."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from alfalfa_amd import build as B
from alfalfa_amd import capi

HIPCC = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc is not installed")

KERNEL = "k_token_workersILb%dELb%dEE"          # <PK, MP> in the mangled name


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """-> {mangled kernel name: {field: int}} of every kernel of parse_kernels.hip"""
    out = str(tmp_path_factory.mktemp("token_kernel") / "parse_kernels.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "parse_kernels.hip"), "-o", out], check=True)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)            # (the kernel's own fields are indented by four, its arguments' deeper)
        if name:
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)(?=\s*\n)", entry + "\n")}
    return kernels


def worker(metadata, packed, per_partition):
    names = [n for n in metadata if KERNEL % (packed, per_partition) in n]
    assert len(names) == 1, names
    return metadata[names[0]]


def test_the_benchmarks_instantiation_uses_no_private_memory(metadata):
    k = worker(metadata, 1, 0)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k


def test_the_other_instantiations_use_no_private_memory_either(metadata):
    for pk, mp in ((0, 0), (1, 1), (0, 1)):
        k = worker(metadata, pk, mp)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (pk, mp, k)


def test_registers_leave_room_for_a_loop_filter_wave(metadata):
    """512 registers per lane of a SIMD; a loop-filter wave takes 256; DESIGN.md 4.5 budgets about 245 for a worker wave"""
    k = worker(metadata, 1, 0)
    assert k["vgpr_count"] <= 245, k
    assert k.get("agpr_count", 0) == 0, k
    for pk, mp in ((0, 0), (1, 1), (0, 1)):         # the others: no accumulation registers, inside 256
        o = worker(metadata, pk, mp)
        assert o["vgpr_count"] <= 256 and o.get("agpr_count", 0) == 0, (pk, mp, o)


def test_lds_use_and_the_launch_shape_are_unchanged(metadata):
    """no static LDS (the tables sit at LDS address 0 of the dynamic request); at 1080p a lane takes 1088 bytes (128 of stream ring +
    a slice of 960: 32 of flag ring, three probability planes of 264, 120 + 15 bytes of above-row flags), and the launch is
    30 lanes x 3 workgroups per CU with a request of 33 792 bytes"""
    for pk in (0, 1):
        for mp in (0, 1):
            k = worker(metadata, pk, mp)
            assert k["group_segment_fixed_size"] == 0, (pk, mp, k)
            assert k["max_flat_workgroup_size"] == 64 and k["wavefront_size"] == 64, (pk, mp, k)
    env = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("ALFALFA_AMD_") and k != "ALFALFA_AMD_LIB"}
    try:
        shape = capi.lib()._ZN2aa18token_worker_shapeEjiPiPjS0_
        shape.argtypes = [C.c_uint32, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        shape.restype = None
        lanes, lds, per_cu = C.c_int(), C.c_uint32(), C.c_int()
        lane_bytes = 128 + ((32 + 3 * 264 + 120 + 15 + 15) & ~15)
        assert lane_bytes == 1088
        shape(lane_bytes, 256, C.byref(lanes), C.byref(lds), C.byref(per_cu))
    finally:
        os.environ.update(env)
    assert (lanes.value, lds.value, per_cu.value) == (30, 33792, 3)
    assert 768 + 30 * lane_bytes <= lds.value < 768 + 31 * lane_bytes
