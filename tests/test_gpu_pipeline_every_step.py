"""Every raster of every step of the PIPELINED decode against the reference decoder, on a real MI355X.

bench.py's Pipeline -- key frames handed to the token workers several groups ahead, inter frames a couple, k_token_workers parsing
the next groups while k_recon_intra4 / k_recon_inter4 / k_recon_inter / k_loopfilter_rows4 reconstruct this one, every frame released
as soon as it is consumed, rasters and coefficient chunks recycled in flight, hand-overs put off when memory is short, every frame
index leaving through aa_download_batch_async into a ring of pinned slabs -- is the regime the benchmark's figure comes from, and
bench.py looks at the last timed step only.  Here the same scheduler runs (tests/pipeline_check.py: CheckedPipeline overrides the
delivery leg alone) and every delivered slab is compared byte for byte with what the reference decoder says the frames are: no
tolerance, no sampling, and the count of rasters compared must be steps x streams x frames.

Each case also has to show that it tested what it claims: token workers alive or jobs waiting beside the reconstruction of a step
other than the last (all cases), hand-overs really put off for lack of memory (case d).  What each run observed goes to the file
ALFALFA_AMD_PIPELINE_RECORD names, one JSON line per case (profiles/pipeline_every_step.md is written from it).

A case that fails is not retried; after a case that ended in a device error the cases behind it fail without touching the GPU."""
import pytest

import alfalfa_amd as aa
import pipeline_check as pc

pytestmark = pytest.mark.gpu

# case d: room for this many groups of pictures, as calibrate planned them, + what the reconstruction calls take (the construction of
# test_admission_keeps_the_books_inside_the_limit in test_bench_pipeline.py).  Measured on the MI355X (profiles/pipeline_every_step.md):
# with 2.5 groups the look-ahead of 4 + 2 groups fits and nothing is put off; with 1.75 hand-overs are put off and the run gets through;
# with 1.25 the run made no progress.
CASE_D_MEMORY_GROUPS = 1.75
# case c: with 32 streams the host's cores parse every key frame inside the host share and the token workers have nothing to do; from
# 128 streams on part of every hand-over goes to the GPU's lanes (measured: workers alive after every step but the last)
CASE_C_STREAMS = 128

_device_in_doubt = []


def run(name, *a, **k):
    assert not _device_in_doubt, "not run: case %s ended in a device error, and nothing is started on a GPU in doubt" % _device_in_doubt[0]
    try:
        return pc.run_case(name, *a, **k)
    except aa.AlfalfaError as e:
        if e.kind != "NoMemory":
            _device_in_doubt.append(name)
        raise


def check(result, record, steps):
    context = pc.context_of(record)
    pc.assert_clean_and_complete(result, steps, context)
    assert record["empty_at_the_end"], context
    assert record["overlap_seen"], "the token workers were idle and the queue empty after every step but the last: nothing was parsed beside the reconstruction\n" + context


@pytest.mark.parametrize("coefficients", ["packed", "dense"])
def test_a_cif_bench_shape_every_step(coefficients):
    """The benchmark's shape in small: 48 streams x 6 frames of the reference encoder's output, 8 steps, the default ring of 3 slabs; more
    than 24 streams, so the urgent host route of an empty pipeline and the device route are both taken.  Asked for: key frames 3 groups
    ahead, inter frames 2.  Where calibrate finds that the host's cores take a hand-over's key frames inside the host share (they did on the
    MI355X: CIF key frames are small), Pipeline itself sets the key-frame look-ahead to the inter-frame depth, as it does for bench.py: the
    run then has K = D = 2 and the lanes parse the inter frames; what ran is in the record and in every failure message."""
    result, record = run("a-" + coefficients, "cif_inter_lf", 48, 6, 8, 3, 2, packed=coefficients == "packed")
    check(result, record, 8)
    assert record["coefficients"] == coefficients


@pytest.mark.parametrize("variant", ["packed", "dense", "lane_per_partition", "header_ahead"])
def test_b_subpel_splitmv_golden_altref_under_load(variant):
    """Quarter-pel luma (six-tap), SPLITMV through k_recon_inter, golden / altref, four DCT partitions -- beside resident workers; once more
    with a lane per partition, once more with the macroblock-header pass a group ahead of the token pass (launch_tokens).  (That the streams
    contain all of it: test_pipeline_check.py::test_the_subpel_case_contains_what_it_is_for.)  Look-ahead as in case a: 3 / 2 asked for, 2 / 2
    where the host takes the key frames.  That the variant was in force is read back: lane_per_partition from the context's info, and
    launch_tokens must have been called in the header_ahead variant and in no other."""
    result, record = run("b-" + variant, "cif_inter_lf_subpel", 48, 6, 6, 3, 2, packed=variant != "dense", lane_per_partition=variant == "lane_per_partition",
                         header_ahead=1 if variant == "header_ahead" else 0)
    check(result, record, 6)
    assert record["lane_per_partition"] == (variant == "lane_per_partition"), "aa_ctx_get_info says lane_per_partition = %s" % record["lane_per_partition"]
    assert record["coefficients"] == ("dense" if variant == "dense" else "packed")
    assert (record["launch_tokens_calls"] > 0) == (variant == "header_ahead"), "launch_tokens was called %d times" % record["launch_tokens_calls"]


def test_c_720p_all_key_frames_every_step():
    """The longest chains there are, and k_recon_intra4 beside resident workers: 128 streams x 4 key frames of 1280x720, 4 steps."""
    result, record = run("c", "720p_intra", CASE_C_STREAMS, 4, 4, 3, 2)
    check(result, record, 4)


def test_d_1080p_short_of_memory_every_step():
    """The headline geometry with hand-overs put off: 64 streams (16 distinct) x 12 frames of 1920x1080, 5 steps, key frames 4 groups ahead,
    inter frames 2 (key frames on the GPU's lanes here), inside a memory limit of CASE_D_MEMORY_GROUPS planned groups, set after calibrate
    (it is computed from what calibrate planned): admission by the planner (Pipeline._room puts hand-overs off), chunk and raster recycling
    while other groups are in flight.  What this does NOT reach: the limit is lowered after the context's first submit, so the coefficient
    heap keeps the size it got under the first limit, and on the MI355X every refusal was the planner's -- refused_by_the_library 0,
    nomem_retries 0: the library's own AA_ERR_NO_MEMORY hand-backs were not taken.  The condition asserted is refused > 0 or nomem_retries > 0."""
    result, record = run("d", "1080p_inter_lf", 64, 12, 5, 4, 2, distinct=16, memory_groups=CASE_D_MEMORY_GROUPS)
    check(result, record, 5)
    assert record["refused"] > 0 or record["nomem_retries"] > 0, "the memory limit of %d bytes (%.1f groups) never bit\n%s" % (
        record["memory_limit"], CASE_D_MEMORY_GROUPS, pc.context_of(record))


def test_e_ring_of_twenty_slabs_trusts_download_wait_alone():
    """More destination slabs than the library has gather buffers (kBindBufs = 16): the checker looks at a slab after
    download_wait(ring - 1) and nothing else, so a download that is counted as arrived while its copy still runs shows as a stale slab
    (aa_download_batch_async waits for a buffer's previous copy before the buffer's index leaves the in-flight list)."""
    result, record = run("e", "cif_inter_lf", 48, 6, 8, 3, 2, ring=20)
    check(result, record, 8)
