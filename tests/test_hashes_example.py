"""examples/ivf_hashes (several IVF files in lock step, one Decoder::prefetch_hashes per frame index, the line `cout << player` prints in
the reference per file and frame) and the C++ shim's Decoder::prefetch_hashes against decoders that never prefetched; built with
plain g++ and -Werror as the other examples are."""
import json
import os
import subprocess

import pytest

import test_cpp_mirror as cm
from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu

HASHES = json.load(open(os.path.join(GOLDEN_DIR, "hash_golden.json")))
NAMES = ["synth_33x17_s7", "qcif_q30_lf24", "synth_175x143_s3"]       # segmentation on and off, 1 to 3 distinct references, 10 / 6 / 6 frames


def test_ivf_hashes_prints_the_references_decoder_hashes():
    exe = cm.build_example("ivf_hashes")
    files = [os.path.join(GOLDEN_DIR, n + ".ivf") for n in NAMES]
    out = subprocess.run([exe] + files, check=True, capture_output=True, timeout=120).stdout.decode()
    want = []
    for t in range(max(len(HASHES[n]["hash"]) for n in NAMES)):
        for n, path in zip(NAMES, files):
            g = HASHES[n]
            if t < len(g["hash"]):
                # DecoderHash::str (decoder.cc:482-490): the hash of the four, then the four
                want.append("%s %d %x (%x_%x_%x_%x)" % (path, t, g["hash"][t], g["state"][t], g["last"][t], g["golden"][t], g["alternative"][t]))
    assert out.splitlines() == want
    assert subprocess.run([exe], capture_output=True).returncode != 0


def test_prefetch_hashes_equals_decoders_that_never_prefetched():
    exe = cm.build_exe(os.path.join(ROOT, "tests", "cpp", "prefetch_hashes_check.cc"), "prefetch_hashes_check")
    files = [os.path.join(GOLDEN_DIR, n + ".ivf") for n in ("synth_64x64_s20", "qcif_q30")]
    r = subprocess.run([exe] + files, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode().strip() == "8 frame indices equal"
