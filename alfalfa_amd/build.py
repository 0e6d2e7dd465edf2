"""Builds the in-tree native library (HIP kernels + host parser + C ABI) for gfx950 with hipcc.

    python -m alfalfa_amd.build          # -> alfalfa_amd/lib/libalfalfa_amd.so

hipcc cross-compiles without a GPU.  The .so is a build product (git-ignored): build() makes it in every fresh tree.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib", "libalfalfa_amd.so")
SOURCES = ["parser.cpp", "runtime.cpp", "kernels.hip", "parse_kernels.hip", "quality_kernels.hip", "hash_kernels.hip", "rebase_kernels.hip", "rebase_compact_kernels.hip", "reencode_kernels.hip", "reencode_compact_kernels.hip", "encode_kernels.hip", "encode_two_pass_kernels.hip", "estimate_kernels.hip", "serializer.cpp", "serialize_kernels.hip", "lf_search_kernels.hip"]
HEADERS = ["parser.hh", "bool_reader.hh", "parse_common.hh", "tok_fsm.hh", "coeff_pack.hh", "recon_inl.hh", "runtime_types.inc", "runtime_pool.inc", "runtime_tokens.inc", "runtime_records.inc", "runtime_ctx.inc", "runtime_submit.inc", "runtime_decode.inc", "runtime_rasters.inc", "runtime_hashes.inc", "runtime_quality.inc", "runtime_lf_search.inc", "runtime_lf_batch.inc", "lf_choose.hh", "runtime_rebase.inc", "runtime_reencode.inc", "runtime_encode.inc", "runtime_estimate.inc", "estimate_size.hh", "qi_choose.hh", "trellis_quant.hh", "key2_first_pass.hh", "runtime_serialize.inc", "serializer.hh", "serialize_common.hh", "bool_writer.hh", "rebase_inl.hh", "rebase_compact.hh", "reencode_compact.hh", "compact_device.hh", "reencode_search.hh", "reencode_mb.hh", "reencode_wave.hh", "reencode_walk.inc", "cost_tables.h", "vp8_tables.h", "vp8_math.hh", "hash_chain.hh", "device_types.h",
           os.path.join("..", "..", "include", "alfalfa_amd.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function"]


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def build(force=False, verbose=False):
    if not force and not stale():
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    cmd = [HIPCC] + FLAGS + os.environ.get("AA_EXTRA_FLAGS", "").split() + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    print(LIB)
