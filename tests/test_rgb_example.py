"""examples/ivf_to_rgb (vp8play's loop without a window: every shown frame as raw rgb24, converted on the GPU through the C++
shim's render_rgb), built with plain g++ as the other examples are, plus the HIP runtime for its device buffer."""
import os
import subprocess

import numpy as np
import pytest

import rgb_reference as rr
from conftest import GOLDEN, GOLDEN_DIR, ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


def build_ivf_to_rgb():
    from alfalfa_amd import build as b
    b.build()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "examples", "ivf_to_rgb.cc")
    exe = os.path.join(BUILD, "ivf_to_rgb")
    hdr = os.path.join(ROOT, "include", "alfalfa_amd", "alfalfa.hh")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(b.LIB)):
        libdir = os.path.dirname(b.LIB)
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(b.HIPCC)))
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__", src, "-o", exe,
                        "-L" + libdir, "-lalfalfa_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                        "-Wl,-rpath," + libdir + ":" + os.path.join(rocm, "lib")], check=True)
    return exe


def test_ivf_to_rgb_builds_and_fails_loudly_without_gpu():
    from alfalfa_amd import capi
    exe = build_ivf_to_rgb()
    assert subprocess.run([exe], capture_output=True).returncode != 0
    assert subprocess.run([exe, "/nonexistent.ivf"], capture_output=True).returncode != 0
    if capi.device_count() == 0:
        r = subprocess.run([exe, os.path.join(GOLDEN_DIR, "qcif_q30.ivf")], capture_output=True)
        assert r.returncode != 0 and b"no HIP device" in r.stderr and r.stdout == b""


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qcif_q30_lf24", "synth_175x143_s3"])
def test_ivf_to_rgb_equals_the_restatement(tmp_path, name):
    import alfalfa_amd as aa
    exe = build_ivf_to_rgb()
    path = os.path.join(GOLDEN_DIR, name + ".ivf")
    out = tmp_path / "o.rgb"
    subprocess.run([exe, "-o", str(out), path], check=True)
    stdout = subprocess.run([exe, path], check=True, capture_output=True).stdout
    w, h, frames = aa.read_ivf(path)
    assert (w, h) == (GOLDEN[name]["width"], GOLDEN[name]["height"])
    d = aa.Decoder(aa.Context(0), w, h)
    want = b""
    for fr in frames:
        shown, fi = d.get_frame_output(fr)
        if shown:
            want += rr.expected(d.raster(fi), w, h, "rgb24").tobytes()
    got = out.read_bytes()
    assert len(got) == len(want) and len(want) % (w * h * 3) == 0
    assert got == want and stdout == want
    assert np.frombuffer(got, np.uint8).size > 0
