"""The second pass's kernels (k_key2_first_pass, k_key2_updates, k_encode_key2; needs a real MI355X) against the reference over the sweep of
tests/golden/two_pass_crafted/sweep.json: 64x64 pictures of tools/make_y4m.crafted that a seeded hunt found to meet at least one of the
three cases no clip of synth_frames reaches -- a Y2 block emptied by check_reset_y2, B_PRED chosen after a 16x16 mode of the first pass, a
first-pass Y2 flag that is set under a B_PRED macroblock -- each with the SHA-256 of the key-frame records xc-enc --two-pass wrote
(tests/golden/make_two_pass_crafted_golden.py, which also held the host model to every one of them).  All tuples go through ONE
encode_frames( two_pass=True ) call, qualities alternating; every job's records must give the stored digest, and the first pass's
token_prob_update must be the host model's.  All comparisons are exact.  The same on the host: tests/test_encode2_sim.py."""
import numpy as np
import pytest

import alfalfa_amd as aa
import encode_model as em
import rebase_model as rm
import two_pass_model as tp
from test_encode_sim import differences
from test_gpu_rebase import device_target

pytestmark = pytest.mark.gpu


def sweep_jobs(ctx):
    """-> (decoders, headers, targets, qualities) of the sweep's tuples, one fresh decoder each; the headers as the 560x288 test makes its own"""
    s = tp.sweep()
    template = tp.case("80x80_q45")["frames"][0]["header"]
    headers = [em.header_like(template, s["width"], s["height"], t["q_index"], key=True) for t in s["tuples"]]
    targets = [device_target(ctx, tp.sweep_target(t)) for t in s["tuples"]]
    return [aa.Decoder(ctx, s["width"], s["height"]) for _ in s["tuples"]], headers, targets, [t["quality"] for t in s["tuples"]]


def check_digests(label, records):
    """records: per tuple (mb, blocks).  Every digest is the stored one; where not, the message is the difference from the host model,
    which gives the stored digest (test_encode2_sim), by tuple and macroblock."""
    from test_encode2_sim import sim_sweep
    tuples = tp.sweep()["tuples"]
    assert len(records) == len(tuples)
    bad = []
    for i, (t, (mb, blocks)) in enumerate(zip(tuples, records)):
        dense = rm.dense(mb, blocks)
        if tp.records_digest(mb, dense) != t["sha256"]:
            smb, sdense = sim_sweep()[i][:2]
            bad.append("tuple %d %s:\n%s" % (i, {k: t[k] for k in ("q_index", "quality") + tp.CRAFTED_ARGS}, "\n".join(differences(mb, dense, smb, sdense)[:4])))
    assert not bad, "%s: %d of %d tuples differ from the reference's records\n%s" % (label, len(bad), len(tuples), "\n".join(bad[:6]))


def check_updates(label, updates):
    from test_encode2_sim import sim_sweep
    for i, (u, want) in enumerate(zip(updates, sim_sweep())):
        wrong = np.flatnonzero(u != want[2])
        assert u.shape == (2112,) and len(wrong) == 0, "%s: tuple %d %s: the first pass's token_prob_update differs from the host model's at %s" % (
            label, i, tp.sweep()["tuples"][i], wrong[:8].tolist())


def test_every_tuple_of_the_sweep_in_one_call_gives_the_reference_s_records(gpu_ctx):
    try:
        for slots in (16, 2):
            gpu_ctx.set_reencode_slots(slots)
            decs, headers, targets, qualities = sweep_jobs(gpu_ctx)
            out = gpu_ctx.encode_frames(decs, headers, targets, quality=qualities, two_pass=True)
            label = "%d macroblocks per round" % slots
            assert all(fi == 0 for fi, _, _, _ in out), label
            check_digests(label, [(mb, blocks) for _, mb, blocks, _ in out])
            check_updates(label, [u for _, _, _, u in out])
    finally:
        gpu_ctx.set_reencode_slots(16)


def test_records_kept_on_the_device_give_the_same_digests(gpu_ctx):
    decs, headers, targets, qualities = sweep_jobs(gpu_ctx)
    out = gpu_ctx.encode_frames(decs, headers, targets, quality=qualities, two_pass=True, records=False)
    records = []
    for d, (fi, nblocks, _) in zip(decs, out):
        _, mb, blocks = d.read_records(fi)
        assert fi == 0 and len(blocks) == nblocks
        records.append((mb, blocks))
    check_digests("records kept on the device", records)
    check_updates("records kept on the device", [u for _, _, u in out])
