"""The model of the probability passes (tests/serialize_model.py) against the frames the reference wrote: for every frame of every
rebased.ivf of tests/golden/rebase and tests/golden/reencode -- made by Encoder::update_residues / reencode_as_interframe, whose last
steps are those passes -- the header's token probability updates, prob_skip_false and the three reference probabilities are what the
model makes of the frame's records and the tables before it, and the tables after the frame follow.  And the census of the fixtures:
updates in each of the three counted planes, a frame without any, the Y2 plane never.  CPU only."""
import numpy as np
import pytest

import alfalfa_amd as aa
import rebase_model as rm
import reencode_model as rmm
import serialize_model as sm

CHUNKS = [("rebase", n) for n in rm.CASES] + [("reencode", n) for n in rmm.CASES]
_seen = {}


def frames_of(kind, name):
    """-> [(header, ext, tables before, tables after, mb, blocks)] of rebased.ivf; made once."""
    if (kind, name) not in _seen:
        case = (rm if kind == "rebase" else rmm).load_case(name)
        p = aa.Parser(case["w"], case["h"])
        p.deserialize_state(rm.decoder_state(case))
        out = []
        for fr in case["rebased"]:
            before = p.probs().copy()
            hdr, mb, blocks = p.parse(fr)
            out.append((hdr, p.header_ext(), before, p.probs().copy(), mb, blocks))
        _seen[kind, name] = out
    return _seen[kind, name]


@pytest.mark.parametrize("kind,name", CHUNKS)
def test_the_reference_s_header_is_what_the_model_makes_of_the_records(kind, name):
    for k, (hdr, ext, before, after, mb, blocks) in enumerate(frames_of(kind, name)):
        what = "%s %s frame %d" % (kind, name, k)
        counts = sm.branch_counts(mb, blocks)
        assert not counts[sm.Y2].any()
        update, values, table = sm.token_updates(counts, before)
        assert (update == np.array(ext["token_prob_update"], bool)).all(), "%s: the model updates other probabilities than the reference" % what
        assert (values == np.array(ext["token_prob"], np.uint8)).all(), "%s: other values" % what
        skip, inter, last, golden = sm.frame_probs(mb)
        assert ext["skip_enabled"] == 1 and ext["prob_skip_false"] == skip, what
        for got, want, field in ((inter, ext["prob_inter"], "prob_inter"), (last, ext["prob_references_last"], "prob_references_last"), (golden, ext["prob_references_golden"], "prob_references_golden")):
            assert got == 0 or got == want, "%s: %s is %d, the model says %d" % (what, field, want, got)
        want_after = table if ext["refresh_entropy_probs"] else before[:1056]
        assert (after[:1056] == want_after).all(), "%s: the tables after the frame are not model( counts, tables before )" % what


def test_the_census_of_the_fixtures():
    """Frames with an update in each of the three counted planes, frames in which a counted plane gets none, the Y2 plane never.  (No
    frame of the fixtures is without ANY update: all 63 update a chroma probability -- the census says so instead of hiding it.)"""
    planes = {sm.Y_AFTER_Y2: 0, sm.Y2: 0, sm.UV: 0, sm.Y_WITHOUT_Y2: 0}
    frames = without_some = without_any = 0
    for kind, name in CHUNKS:
        for hdr, ext, *_ in frames_of(kind, name):
            up = np.array(ext["token_prob_update"], bool).reshape(4, -1)
            for t in planes:
                planes[t] += bool(up[t].any())
            frames += 1
            without_some += not all(up[t].any() for t in (sm.Y_AFTER_Y2, sm.UV, sm.Y_WITHOUT_Y2))
            without_any += not up.any()
    assert planes[sm.Y_AFTER_Y2] and planes[sm.UV] and planes[sm.Y_WITHOUT_Y2], planes
    assert planes[sm.Y_AFTER_Y2] < frames and planes[sm.Y_WITHOUT_Y2] < frames and without_some, (planes, frames)
    assert planes[sm.Y2] == 0
    assert (frames, without_any) == (63, 0)
