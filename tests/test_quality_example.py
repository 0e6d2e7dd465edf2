"""examples/ivf_ssim (xc-ssim's loop for two IVF files, scored on the GPU through the C++ shim's quality_batch) and the shim's
RasterHandle::quality, built with plain g++ and -Werror as the other examples are."""
import os
import subprocess

import pytest

import vp8_oracle as vo
import test_cpp_mirror as cm
from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu

FILES = [os.path.join(GOLDEN_DIR, n + ".ivf") for n in ("qcif_q30", "qcif_q30_lf24")]


def shown_planes(path):
    """-> the padded planes of every shown frame, decoded by the oracle."""
    w, h, frames = vo.read_ivf(path)
    ora = vo.OracleDecoder(w, h)
    return [ora.planes() for fr in frames if ora.decode(fr)]


def six_digits(x):
    """What an ostream prints for a double by default (%g: 6 significant digits), read back."""
    return float("%g" % x)


@pytest.mark.parametrize("all_planes", [False, True])
def test_ivf_ssim_prints_the_oracles_values(all_planes):
    exe = cm.build_example("ivf_ssim")
    out = subprocess.run([exe] + (["-a"] if all_planes else []) + FILES, check=True, capture_output=True).stdout.decode()
    a, b = shown_planes(FILES[0]), shown_planes(FILES[1])
    lines = out.splitlines()
    assert len(lines) == min(len(a), len(b)) > 0
    for i, line in enumerate(lines):
        got = [float(x) for x in line.split("\t")]
        want = [six_digits(vo.ssim_plane(p.tobytes(), q.tobytes(), p.shape[1], p.shape[0])) for p, q in zip(a[i], b[i])]
        assert got == (want if all_planes else want[:1]), "frame %d: %r" % (i, line)
    assert subprocess.run([exe], capture_output=True).returncode != 0
    assert subprocess.run([exe, FILES[0]], capture_output=True).returncode != 0


def test_the_shorter_file_ends_the_loop(tmp_path):
    exe = cm.build_example("ivf_ssim")
    short = os.path.join(GOLDEN_DIR, "qcif_allkey_q20.ivf")            # 4 frames against 6
    n_short, n_long = len(shown_planes(short)), len(shown_planes(FILES[0]))
    assert n_short < n_long
    for pair in ([short, FILES[0]], [FILES[0], short]):
        out = subprocess.run([exe] + pair, check=True, capture_output=True).stdout.decode()
        assert len(out.splitlines()) == n_short


def test_raster_handle_quality_equals_the_host_measure_of_the_downloads():
    exe = cm.build_exe(os.path.join(ROOT, "tests", "cpp", "quality_handles.cc"), "quality_handles")
    r = subprocess.run([exe] + FILES, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode().strip() == "%d pairs equal" % len(shown_planes(FILES[0]))
