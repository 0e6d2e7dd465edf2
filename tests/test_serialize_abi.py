"""The serialisation's entry points without a GPU: the symbols are exported and bound (the ABI version stays what it was: they are additions, no existing struct or call changed), aa_frame_header_ext has the
layout the bindings mirror, and the header a parser hands out (aa_parser_last_header_ext) is complete: with the tables before a frame it
gives the tables after it, for every frame of every stream of tests/golden."""
import ctypes as C
import glob
import os
import re

import numpy as np

import alfalfa_amd as aa
from alfalfa_amd import capi
from conftest import GOLDEN_DIR

NEW = ["aa_serialize_host", "aa_serialize_batch", "aa_serialize_last_timing", "aa_parser_last_header_ext", "aa_stream_last_header_ext", "aa_parser_last_sub_modes", "aa_stream_last_sub_modes"]


def test_the_entry_points_are_exported_and_the_version_is_the_header_s():
    L = capi.lib()
    bound = {n for n, _, _ in capi.SYMBOLS}
    for n in NEW:
        assert hasattr(L, n) and n in bound, n
    version = int(re.search(r"#define AA_ABI_VERSION (\d+)", open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "alfalfa_amd.h")).read()).group(1))
    assert L.aa_abi_version() == version == 4
    text = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "alfalfa_amd.h")).read()
    assert all(n + "(" in text for n in NEW)


def test_struct_layouts():
    assert C.sizeof(capi.FrameHeaderExt) == 2258 and C.alignment(capi.FrameHeaderExt) == 1
    assert capi.FrameHeaderExt.token_prob_update.offset == 2258 - 2112 and capi.FrameHeaderExt.mv_prob_update.offset == 2258 - 2112 - 76
    assert C.sizeof(capi.SerializeJob) == 96 and capi.SerializeJob.size.offset == 80 and capi.SerializeJob.counts_out.offset == 88


def test_null_arguments_are_refused_without_a_device():
    L = capi.lib()
    assert L.aa_serialize_batch(None, None, 0) == -7
    assert L.aa_parser_last_header_ext(None, None) == -7
    n = C.c_size_t()
    assert L.aa_parser_last_sub_modes(None, None, 0, C.byref(n)) == -7


def test_the_parsed_header_is_complete():
    streams = sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.ivf")))
    assert len(streams) >= 10
    seen = {"token": 0, "mv": 0, "ymode": 0, "no_refresh": 0, "seg_map": 0, "sub_modes": 0}
    for path in streams:
        w, h, frames = aa.read_ivf(path)
        p = aa.Parser(w, h)
        assert p.header_ext() == capi.FrameHeaderExt().as_dict()
        for k, fr in enumerate(frames):
            before = p.probs().copy()
            hdr, mb, _ = p.parse(fr)
            x = p.header_ext()
            t = before.copy()
            if hdr["key_frame"]:
                q = aa.Parser(w, h)
                t = q.probs().copy()          # the defaults
            up, val = np.array(x["token_prob_update"], bool), np.array(x["token_prob"], np.uint8)
            t[:1056][up] = val[up]
            if not hdr["key_frame"]:
                if x["intra_16x16_update"]:
                    t[1056:1060] = x["intra_16x16_prob"]
                if x["intra_chroma_update"]:
                    t[1060:1063] = x["intra_chroma_prob"]
                mu, mv = np.array(x["mv_prob_update"], bool), np.array(x["mv_prob"], np.int32)
                t[1063:][mu] = np.where(mv[mu] > 0, mv[mu] << 1, 1)
            else:
                assert not any(x["mv_prob_update"]) and x["prob_inter"] == 0
            after = p.probs()
            if x["refresh_entropy_probs"] or hdr["key_frame"]:
                want = t if x["refresh_entropy_probs"] else aa.Parser(w, h).probs()
                assert (after == want).all(), "%s frame %d: tables before + header updates are not the tables after" % (path, k)
            else:
                assert (after == before).all()
            subs = p.sub_modes()
            splits = mb[mb["y_mode"] == 9]
            assert len(subs) == sum((2, 2, 4, 16)[s] for s in splits["split_partition"]) and all(10 <= m <= 13 for m in subs)
            seen["token"] += bool(up.any()); seen["mv"] += bool(any(x["mv_prob_update"])); seen["ymode"] += x["intra_16x16_update"]
            seen["no_refresh"] += not x["refresh_entropy_probs"]; seen["seg_map"] += x["update_mb_segmentation_map"]; seen["sub_modes"] += len(subs) > 0
    assert all(seen.values()), seen
