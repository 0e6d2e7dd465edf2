"""The two-pass encoder's part of the C ABI: the symbols include/alfalfa_amd.h declares for it are exported and bound, the prototypes
stand in the header, the existing structures keep their sizes, and what the calls refuse without a device.  CPU only."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import alfalfa_amd as aa
from alfalfa_amd import capi
from conftest import ROOT
from test_capi import declared_symbols

NEW = ["aa_encode_two_pass_batch", "aa_encode_two_pass_device_batch", "aa_serialize_two_pass_batch"]


def test_the_new_symbols_are_declared_exported_and_bound():
    L = capi.lib()
    declared, bound = declared_symbols(), {n for n, _, _ in capi.SYMBOLS}
    for n in NEW:
        assert n in declared and hasattr(L, n) and n in bound, n


def test_the_prototypes_stand_in_the_header_and_no_structure_changed():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "alfalfa_amd.h")).read())
    for line in ("#define AA_TWO_PASS_UPDATES 2112",
                 "aa_status aa_encode_two_pass_batch( aa_ctx * ctx, aa_encode_job * jobs, int n, const uint8_t * two_pass, uint8_t * first_pass_updates );",
                 "aa_status aa_encode_two_pass_device_batch( aa_ctx * ctx, aa_encode_device_job * jobs, int n, const uint8_t * two_pass, uint8_t * first_pass_updates );",
                 "aa_status aa_serialize_two_pass_batch( aa_ctx * ctx, aa_serialize_job * jobs, int n, const uint8_t * first_pass_updates );"):
        assert line in text, line
    assert capi.TWO_PASS_UPDATES == 2112
    assert C.sizeof(capi.EncodeJob) == 96 and C.sizeof(capi.EncodeDeviceJob) == 16 + 40 + 4 + 12 and C.sizeof(capi.SerializeJob) == 96
    assert "#define AA_ABI_VERSION 4" in text and capi.lib().aa_abi_version() == 4          # (an addition: the version stands)


def test_refusals_that_need_no_device():
    L = capi.lib()
    jobs, djobs, sjobs = (capi.EncodeJob * 1)(), (capi.EncodeDeviceJob * 1)(), (capi.SerializeJob * 1)()
    flags, updates = np.ones(1, np.uint8), np.zeros(2112, np.uint8)
    f, u = flags.ctypes.data_as(C.c_void_p), updates.ctypes.data_as(C.c_void_p)
    assert L.aa_encode_two_pass_batch(None, jobs, 1, None, u) == -7 and L.aa_last_error().startswith(b"aa_encode_two_pass_batch:")
    assert L.aa_encode_two_pass_batch(None, jobs, 1, f, None) == -7
    assert L.aa_encode_two_pass_batch(None, jobs, 1, f, u) == -7 and L.aa_last_error().startswith(b"aa_encode_batch:")      # (from here on the call is aa_encode_batch's)
    assert L.aa_encode_two_pass_device_batch(None, djobs, 1, None, u) == -7 and L.aa_last_error().startswith(b"aa_encode_two_pass_device_batch:")
    assert L.aa_encode_two_pass_device_batch(None, djobs, 0, f, u) == -7
    assert L.aa_serialize_two_pass_batch(None, sjobs, 1, None) == -7 and L.aa_last_error().startswith(b"aa_serialize_two_pass_batch:")
    assert L.aa_serialize_two_pass_batch(None, sjobs, 1, u) == -7 and L.aa_last_error().startswith(b"aa_serialize_batch:")


def test_the_python_calls_take_the_new_arguments_and_default_to_the_old_behaviour():
    for fn, arg in ((aa.Context.encode_frames, "two_pass"), (aa.Decoder.encode_frame, "two_pass")):
        assert inspect.signature(fn).parameters[arg].default is False
    for fn in (aa.Context.serialize_frames, aa.Decoder.serialize_frame):
        assert inspect.signature(fn).parameters["first_pass_updates"].default is None
