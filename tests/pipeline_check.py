"""bench.py's Pipeline with EVERY delivered raster of EVERY step compared with the reference decoder.

bench.py itself compares the rasters of the last timed step (frames 0, F/2, F-1 of the distinct streams); every other step's output
is released unseen.  CheckedPipeline is the same scheduler -- nothing about what is handed over, or when, differs -- whose delivery
leg looks at each pinned slab after the wait the base class already issues and before the slab is handed to the next download:
    expected_rasters()   what the reference decoder (oracle/_ref/ref_decode), or the oracle, says every frame of every distinct stream is
    CheckedPipeline      bench.Pipeline with _deliver overridden: memory compare of the slab's previous content, stream by stream
    make_case_env()      bench.make_env for a test case (streams generated with a bounded worker count, a few distinct seeds repeated)
    run_case()           one GPU case in a context of its own: make_env -> calibrate -> CheckedPipeline.run -> finish -> a record dict
    assert_clean_and_complete()   no mismatch, and exactly steps * S * F rasters compared
A plain module: tests/test_pipeline_check.py drives it against a fake context on the CPU, tests/test_gpu_pipeline_every_step.py on the GPU."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import tempfile
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import ROOT

REF_DECODE = os.path.join(ROOT, "oracle", "_ref", "ref_decode")
MAX_WORKERS = 16                      # stream generation and the reference decodes: never sized by os.cpu_count() alone


def load_bench():
    """bench.py as a module (it is a script at the repository's root, not part of the package)."""
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bench = load_bench()


def workers():
    return max(1, min(MAX_WORKERS, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))


def padded_geometry(width, height):
    return (width + 15) // 16 * 16, (height + 15) // 16 * 16


def _reference_frames(path, F, tmpdir):
    raw = os.path.join(tmpdir, "ref_%d_%s.raw" % (os.getpid(), os.path.basename(path)))
    subprocess.run([REF_DECODE, path, raw], check=True, stdout=subprocess.DEVNULL)
    data = np.fromfile(raw, np.uint8)
    os.unlink(raw)
    assert len(data) % F == 0 and len(data) > 0, (path, len(data), F)
    return data.reshape(F, len(data) // F)


def _oracle_frames(path, F):
    import vp8_oracle as vo
    w, h, frames = vo.read_ivf(path)
    assert len(frames) == F, (path, len(frames), F)
    ora = vo.OracleDecoder(w, h)
    out = []
    for fr in frames:
        ora.decode(fr)
        out.append(np.frombuffer(ora.raster_bytes(), np.uint8))
    return np.stack(out)


def expected_rasters(paths, F, cross_check=False):
    """-> ([uint8 array [F, raster bytes] per path], source).  Each row is a frame's three padded planes back to back: what
    Decoder.raster_bytes and an entry of a delivered slab hold.  Source of truth: the reference decoder built in place
    (oracle/_ref/ref_decode) where it is there, else the oracle.  cross_check (the synthetic streams, which no encoder of the
    reference wrote): where both are there they must agree before either is used."""
    have_ref = os.path.exists(REF_DECODE)
    with ThreadPoolExecutor(max_workers=workers()) as ex, tempfile.TemporaryDirectory() as td:
        if have_ref:
            out = list(ex.map(lambda p: _reference_frames(p, F, td), paths))
            source = "oracle/_ref/ref_decode"
            if cross_check:
                for p, a, b in zip(paths, out, ex.map(lambda p: _oracle_frames(p, F), paths)):
                    assert a.shape == b.shape and np.array_equal(a, b), "the reference decoder and the oracle disagree on %s" % os.path.basename(p)
                source += " (agrees with vp8_oracle.OracleDecoder)"
        else:
            out = list(ex.map(lambda p: _oracle_frames(p, F), paths))
            source = "vp8_oracle.OracleDecoder (oracle/_ref/ref_decode is not built)"
    return out, source


def locate(offset, pw, ph):
    """Byte offset in a raster (Y, U, V padded planes back to back) -> (plane, x, y): the arithmetic of first_diff in test_gpu_parity.py."""
    if offset < pw * ph:
        return 0, offset % pw, offset // pw
    csz, cw = pw * ph // 4, pw // 2
    o2 = (offset - pw * ph) % csz
    return 1 + (offset - pw * ph) // csz, o2 % cw, o2 // cw


class CheckedPipeline(bench.Pipeline):
    """bench.Pipeline whose delivered frames are all compared.  `expected[k]` is the [F, raster bytes] array of distinct stream k,
    `which[i]` the distinct stream that stream i of the list is.  Only _deliver differs from the base class."""
    MAX_REPORTED = 48

    def __init__(self, env, stream_list, key_ahead, depth, header_ahead=0, expected=None, which=None):
        super().__init__(env, stream_list, key_ahead, depth, header_ahead)
        self.expected, self.which = expected, list(which)
        assert len(self.which) == self.n and all(e.shape == (self.F, env["raster_bytes"]) for e in expected)
        self.pw, self.ph = padded_geometry(env["width"], env["height"])
        assert self.pw * self.ph * 3 // 2 == env["raster_bytes"]
        ring = env["deliver_ring"]
        nbytes = self.n * env["raster_bytes"]
        self.views = [np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(a)).reshape(self.n, env["raster_bytes"]) for a in ring]
        self.slab_holds = [None] * len(ring)      # slab -> (group, frame) of the download queued into it last and not compared yet
        self.compared = 0                         # rasters compared
        self.bad_rasters = 0
        self.mismatches = []                      # (group, frame, stream, plane, x, y, got, want): the first differing byte of a bad raster
        self.details = []                         # one line per entry of mismatches: how many bytes differ, which luma rows, which slab
        self.bad_slabs = set()
        self.check_s = 0.0

    def _check_slab(self, k):
        held = self.slab_holds[k]
        if held is None:
            return
        t = time.perf_counter()
        g, f = held
        view = self.views[k]
        for i in range(self.n):
            want = self.expected[self.which[i]][f]
            if not np.array_equal(view[i], want):
                self.bad_rasters += 1
                self.bad_slabs.add(k)
                if len(self.mismatches) < self.MAX_REPORTED:
                    got = view[i].copy()
                    bad = np.nonzero(got != want)[0]
                    if not len(bad):          # (it differed a moment ago and no longer does: a copy was still writing the slab)
                        self.mismatches.append((g, f, i, -1, -1, -1, -1, -1))
                        self.details.append("group %d frame %d stream %d (slab %d): differed when compared, equal when read again -- a copy was still writing" % (g, f, i, k))
                        continue
                    o = int(bad[0])
                    plane, x, y = locate(o, self.pw, self.ph)
                    self.mismatches.append((g, f, i, plane, x, y, int(got[o]), int(want[o])))
                    luma = bad[bad < self.pw * self.ph] // self.pw
                    self.details.append("group %d frame %d stream %d (slab %d): %d bytes differ, first in plane %d at x=%d y=%d (macroblock row %d) got %d want %d; luma rows %s"
                                        % (g, f, i, k, len(bad), plane, x, y, y // (16 if plane == 0 else 8), got[o], want[o],
                                           "%d..%d" % (luma[0], luma[-1]) if len(luma) else "none"))
        self.compared += self.n
        self.slab_holds[k] = None
        self.check_s += time.perf_counter() - t

    def _deliver(self, ds, f):
        """As the base class: the wait for the copy that used this slab before, then the next download into it -- with the slab's
        previous content compared in between (which group and frame that was is this class's own book)."""
        env = self.env
        ring = env["deliver_ring"]
        k = self.deliveries % len(ring)
        self.deliveries += 1
        self.ctx.download_wait(len(ring) - 1)
        self._check_slab(k)
        self.ctx.download_batch_async(ds, [f] * len(ds), ring[k], env["raster_bytes"])
        self.slab_holds[k] = (self.decoded, f)
        self.delivered_bytes += len(ds) * env["raster_bytes"]

    def finish(self):
        """The end of a run: every download has arrived, and the slabs nobody has looked at yet are compared."""
        self.ctx.download_wait(0)
        for k in range(len(self.slab_holds)):
            self._check_slab(k)


def assert_clean_and_complete(pipe, steps, context=""):
    """No raster differed, and the checker left out nothing: exactly steps * S * F rasters went through the comparison."""
    assert not pipe.mismatches and not pipe.bad_rasters, "%d rasters differ from the reference; first ones (group, frame, stream, plane, x, y, got, want): %r\n%s\n%s" % (
        pipe.bad_rasters, pipe.mismatches[:8], "\n".join(pipe.details[:8]), context)
    assert pipe.compared == steps * pipe.n * pipe.F, "%d rasters compared, %d steps x %d streams x %d frames = %d delivered\n%s" % (
        pipe.compared, steps, pipe.n, pipe.F, steps * pipe.n * pipe.F, context)


def case_args():
    """What bench.parse_args() would give, as far as make_env, calibrate and Pipeline look at it."""
    return types.SimpleNamespace(config="(a test case: no config is the headline one)", trace_memory=False, overcommit=1.2, urgent_groups=2, no_urgent_host=False)


def make_case_env(ctx, config, S, F, distinct=None, threads=None):
    """bench.make_env for S streams of `config`; with `distinct`, S streams drawn in turn from the first `distinct` seeds of the pool
    (100, 101, ...).  The streams are generated first, with a bounded number of workers."""
    import workload
    from alfalfa_amd import sharding
    n = distinct or S
    assert S % n == 0
    seeds = sorted(set(100 + (g - 100) % (8 if workload.CONFIGS[config][2] == "synth" else 24) for g in sharding.stream_ids(0, 1, n)))
    made = set(workload.make_streams(config, F, seeds, workers=workers()))
    env = bench.make_env(case_args(), ctx, config, n, F, 0, 1, threads or workers())
    # (make_env asks for the streams once more, with a pool sized its own way: by now that only looks the files up.  The seeds above
    # restate its pool sizes; if those change, this says so instead of letting make_env generate streams unbounded)
    assert set(env["paths"]) <= made, "bench.make_env drew streams that were not generated beforehand: %r" % sorted(set(env["paths"]) - made)[:4]
    if distinct:
        assert len(env["distinct"]) == n, "the pool has fewer than %d distinct streams of %s" % (n, config)
        rep = S // n
        for key in ("seeds", "paths", "streams"):
            env[key] = env[key] * rep
        env["S"] = S
        env["compressed_bytes"] *= rep
        env["mbs_per_step"] = S * F * env["mbs_per_frame"]
    return env


def overlap_seen(series):
    """In a step other than the last, were token workers alive or jobs waiting when the step's reconstruction had been queued?"""
    return any(alive > 0 or waiting > 0 for _, alive, waiting, *_ in series[:-1])


def write_record(record):
    path = os.environ.get("ALFALFA_AMD_PIPELINE_RECORD")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(record) + "\n")


def run_case(name, config, S, F, steps, key_ahead, depth, ring=None, packed=True, lane_per_partition=False, header_ahead=0, distinct=None,
             memory_groups=None, context_limit=int(32e9)):
    """One case on the GPU, in a context of its own: make_env -> calibrate -> CheckedPipeline.run(steps) from an empty pipeline to an
    empty pipeline -> finish.  memory_groups: after calibrate the context's limit is lowered to room for that many groups of pictures
    as calibrate planned them (+ what the reconstruction calls take).  -> (result, record): the checker's findings (what
    assert_clean_and_complete reads) and the observations; pipeline, ring and context are dropped before returning."""
    import alfalfa_amd as aa
    ring = ring or bench.DELIVER_RING
    t_case = time.perf_counter()
    ctx = aa.Context(0)                      # raises NoDevice without a GPU
    slabs = []
    try:
        ctx.set_packed_coefficients(packed)
        ctx.set_memory_limit(context_limit)
        if lane_per_partition:
            ctx.set_lane_per_partition(True)
        env = make_case_env(ctx, config, S, F, distinct)
        paths = [env["paths"][i] for i in env["distinct"]]
        t0 = time.perf_counter()
        expected, source = expected_rasters(paths, F, cross_check=config.endswith("_subpel"))
        t_expected = time.perf_counter() - t0
        which = [env["distinct"].index(env["seeds"].index(sd)) for sd in env["seeds"]]
        bench.calibrate(env, env["streams"])
        limit = None
        if memory_groups:
            per_group = S * (env["key_coeff_bytes"] + env["key_arena_bytes"] + (F - 1) * (env["inter_coeff_bytes"] + env["inter_arena_bytes"]))
            limit = int(memory_groups * per_group + env["recon_reserve"])
            ctx.set_memory_limit(limit)
        slabs = [ctx.pinned_alloc(S * env["raster_bytes"]) for _ in range(ring)]
        env["deliver_ring"] = slabs
        pipe = CheckedPipeline(env, env["streams"], key_ahead, depth, header_ahead, expected=expected, which=which)
        pipe.step_series = []
        pipe.wait_mark = (0, 0)
        token_launches = []
        launch_tokens = ctx.launch_tokens

        def counted_launch_tokens(n):
            token_launches.append(n)
            return launch_tokens(n)
        ctx.launch_tokens = counted_launch_tokens
        ctx.kernel_stats(reset=True)
        t0 = time.perf_counter()
        error = None
        try:
            pipe.run(steps)
            pipe.finish()
            ctx.sync()
        except aa.AlfalfaError as e:
            error = e
        wall = time.perf_counter() - t0
        stats = ctx.kernel_stats() if error is None or error.kind == "NoMemory" else {}
        record = {"case": name, "config": config, "streams": S, "distinct_streams": len(expected), "frames": F, "steps": steps, "key_ahead": pipe.K, "depth": pipe.D,
                  "header_ahead": header_ahead, "ring": ring, "coefficients": "packed" if ctx.info()["packed_coefficients"] else "dense", "lane_per_partition": bool(ctx.info()["lane_per_partition"]),
                  "launch_tokens_calls": len(token_launches),
                  "wall_s": round(wall, 2), "check_s": round(pipe.check_s, 2), "expected_s": round(t_expected, 2), "case_s": None,
                  "rasters_compared": pipe.compared, "rasters_delivered": steps * S * F, "bad_rasters": pipe.bad_rasters, "mismatches": pipe.mismatches[:8],
                  "details": pipe.details[:8], "bad_slabs": sorted(pipe.bad_slabs), "expected_source": source, "refused": pipe.refused,
                  "refused_by_the_library": pipe.refused_by_the_library, "nomem_retries": stats.get("nomem_retries"),
                  "row_handoff_rereads": stats.get("row_handoff_rereads"), "row_handoff_stale_polls": stats.get("row_handoff_stale_polls"),
                  "frames_parsed_on_host_cores": stats.get("host_routed_frames"),
                  "keys_on_host": bool(env.get("keys_on_host")), "urgent_groups": pipe.urgent_groups, "memory_limit": limit, "memory_groups": memory_groups,
                  "planned": env.get("planned"), "recon_reserve": env.get("recon_reserve"),
                  "empty_at_the_end": pipe.keys == pipe.decoded == pipe.inter_h and not pipe.groups,
                  "per_step_ms_alive_waiting": [list(x[:3]) for x in pipe.step_series], "overlap_seen": overlap_seen(pipe.step_series),
                  "error": None if error is None else str(error)}
        record["case_s"] = round(time.perf_counter() - t_case, 2)
        write_record(record)
        result = types.SimpleNamespace(mismatches=pipe.mismatches, details=pipe.details, bad_rasters=pipe.bad_rasters, compared=pipe.compared, n=pipe.n, F=pipe.F,
                                       refused=pipe.refused, step_series=pipe.step_series)
        pipe.views = None
        del pipe
        if error is not None:
            raise error
        return result, record
    finally:
        try:
            ctx.sync()
        except Exception:
            pass
        for a in slabs:
            ctx.pinned_free(a)


def context_of(record):
    """The part of a failure message that says what the run was and what the hand-off counters saw."""
    return "key frames %d groups ahead, inter frames %d (key frames parsed on the host: %s); expected from %s; row_handoff_rereads %s, row_handoff_stale_polls %s, nomem_retries %s, refused %s; per step [ms, workers alive, jobs waiting]: %s" % (
        record["key_ahead"], record["depth"], record["keys_on_host"], record["expected_source"], record["row_handoff_rereads"], record["row_handoff_stale_polls"], record["nomem_retries"], record["refused"],
        record["per_step_ms_alive_waiting"])
