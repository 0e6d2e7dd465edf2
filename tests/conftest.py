import hashlib
import json
import os
import sys

import pytest

# A decoder context runs 16 HIP streams and wants a hardware queue for each (include/alfalfa_amd.h, aa_runtime_prepare); the
# library keeps whatever value the environment already has.  The suite asks for 16 for itself -- before anything in this process
# starts HIP -- and the programs it starts (bench.py, the C++ callers) inherit it.  A value of 16 or more stands.
try:
    _queues = int(os.environ.get("GPU_MAX_HW_QUEUES") or 0)
except ValueError:
    _queues = 0
if _queues < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"

ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def load_golden():
    return json.load(open(os.path.join(GOLDEN_DIR, "golden.json")))


GOLDEN = load_golden()


def golden_frames(name):
    import vp8_oracle as vo
    w, h, frames = vo.read_ivf(os.path.join(GOLDEN_DIR, name + ".ivf"))
    return w, h, frames


def sha256(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="session", params=["packed", "dense"])
def gpu_ctx(request):
    """The session's shared context, once per coefficient storage format of the device parser: every -m gpu test that takes it
    runs in both (packed is the product's default; dense is what host-parsed frames use and what reconstruction reads)."""
    import alfalfa_amd as aa
    ctx = aa.Context(0)    # raises NoDevice on a box without a GPU: -m gpu tests must not pass silently
    ctx.set_packed_coefficients(request.param == "packed")
    assert ctx.info()["packed_coefficients"] == (1 if request.param == "packed" else 0)
    return ctx
