"""Timing of aa_stream_lf_search on a 1080p stream of the benchmark workload: python tools/lf_search_probe.py

--batch: probe of the batched loop-filter level search (aa_lf_search_decode_batch) instead: the workload of tools/reencode_probe.py --device -- the
benchmark's distinct 1080p streams, 4x over: 480 decoders that have decoded their key frame, each holding the stream's next picture
re-encoded as an inter frame (-q rt) with its records on the device and a provisional level of 63 in its header -- searched over 0..63
and decoded in ONE call.

    python tools/lf_search_probe.py --batch [--streams 120] [--copies 4] [--reps 3] [--baseline 32] [--levels 4] [--out results.json]

Reports, per repetition (a warm-up call before them is not reported): the wall time of the call (a host clock around it; the call ends
in a synchronise) and what aa_lf_search_last_timing says of it between HIP events -- the unfiltered reconstruction, k_lf_candidates, the
candidates' loop filter, the scoring, k_lf_choose with the states coming down, k_lf_finish with the final filter --, the rounds, the
levels chosen, k_lf_candidates' bytes per second (the unfiltered rasters and records read once and written once per candidate of level
> 0) and, with Context.profile on, the loop-filter kernel's own time.  --baseline N: on the first N frames, in the same process and
alternating with the batched call on those N, the only other way to the same levels: every frame serialised, then a loop of
Decoder.lf_search (aa_stream_lf_search: one stream per call, the frame as bytes) over 0..63 -- reported beside it, and the levels
compared.  profiles/lf_search_batch.md holds what was measured."""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import alfalfa_amd as aa  # noqa: E402


def single():
    import workload
    w, h, frames = aa.read_ivf(workload.make_stream("1080p_inter_lf", 4, 100))
    ctx = aa.Context(0)
    dec = aa.Decoder(ctx, w, h)
    for fr in frames[:2]:
        dec.get_frame_output(fr)
    pw, ph = dec.padded_width, dec.padded_height
    orig = np.frombuffer(dec.raster_bytes(1), np.uint8)[:pw * ph].reshape(ph, pw).copy()
    out = {}
    for lo, hi in ((23, 25), (0, 63), (23, 25), (0, 63)):        # (first use pays for the scratch decoders' first-touch allocations)
        t0 = time.perf_counter()
        best, q, qs, _ = dec.lf_search(frames[2], orig, lo, hi)
        out["%d..%d" % (lo, hi)] = {"seconds": round(time.perf_counter() - t0, 4), "best_level": best, "ssim": round(q, 6)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="store_true", help="the batched call on 480 device-resident frames (without it: aa_stream_lf_search on one stream)")
    ap.add_argument("--config", default="1080p_inter_lf")
    ap.add_argument("--streams", type=int, default=120)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline", type=int, default=32, help="frames of the loop of aa_stream_lf_search (0: none)")
    ap.add_argument("--levels", type=int, default=0, help="levels per round (0: the context's default)")
    ap.add_argument("--out", help="also write the results as JSON to this file")
    args = ap.parse_args()
    if not args.batch:
        return single()
    import torch
    import workload

    paths = workload.make_streams(args.config, 2, list(range(100, 100 + args.streams)))
    ctx = aa.Context(0)
    if args.levels:
        ctx.set_lf_search_round(args.levels)
    headers, exts, targets, keys, size = [], [], [], [], None
    for p in paths:
        w, h, frames = aa.read_ivf(p)
        size = (w, h)
        parser = aa.Parser(w, h)
        parser.parse(frames[0])
        hdr, _, _ = parser.parse(frames[1])
        if hdr["segmentation_enabled"]:
            raise SystemExit("lf_search_probe: %s uses segmentation" % p)
        headers.append(dict(hdr, loop_filter_level=63, filter_adjustments_enabled=1)); exts.append(aa.with_zero_lf_deltas(parser.header_ext())); keys.append(frames[0])
        d = aa.Decoder(ctx, w, h)
        d.get_frame_output(frames[0])
        _, fi = d.get_frame_output(frames[1])
        pw, ph = d.padded_width, d.padded_height
        planes = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
        d.export_raster_device(fi, *[t.data_ptr() for t in planes])
        ctx.sync()
        targets.append(tuple(planes))
        del d
    torch.cuda.synchronize()
    n = len(paths) * args.copies
    b_hdr, b_ext, b_t, b_key = headers * args.copies, exts * args.copies, targets * args.copies, keys * args.copies
    raster_bytes = pw * ph * 3 // 2
    record_bytes = 80 * (pw // 16) * (ph // 16)

    def provisional(count):
        """`count` fresh decoders, each with the re-encoded frame appended on the device -> (decoders, frame indices)"""
        decs = []
        for i in range(count):
            d = aa.Decoder(ctx, *size)
            d.get_frame_output(b_key[i])
            decs.append(d)
        results = ctx.reencode_as_inter(decs, b_hdr[:count], b_t[:count], quality="rt", records=False)
        ctx.sync()
        return decs, [r[0] for r in results]

    def batched(count):
        decs, fis = provisional(count)
        ctx.kernel_stats(reset=True)
        t0 = time.perf_counter()
        results = ctx.lf_search_decode(decs, fis, b_t[:count])
        wall = (time.perf_counter() - t0) * 1e3
        timing = ctx.lf_search_timing()
        timing["python_call_ms"] = wall
        timing["loopfilter_kernel_ms"] = ctx.kernel_stats()["loopfilter_ms"]
        # what k_lf_candidates moved: per job and round one read of raster and records, a write per candidate of level > 0
        moved = 0
        K = args.levels or 4
        for _, _, evaluated in results:
            for first in range(0, evaluated, K):
                cands = min(K, 64 - first)
                moved += (raster_bytes + record_bytes) * (1 + cands - (1 if first == 0 else 0))
        timing["candidates_bytes"] = moved
        timing["candidates_bytes_per_s"] = moved / (timing["candidates_ms"] * 1e-3) if timing["candidates_ms"] else 0.0
        levels = [r[0] for r in results]
        del decs
        return timing, levels, [r[2] for r in results]

    def looped(count):
        decs, fis = provisional(count)
        # the parent's route: the records through the host into bytes, then one stream per call
        frames = ctx.serialize_frames(decs, fis, b_hdr[:count], b_ext[:count], optimise=True)
        originals = [b_t[i][0].cpu().numpy() for i in range(count)]
        before = []                                      # decoders that stand where the frames' streams stood before them
        for i in range(count):
            d = aa.Decoder(ctx, *size)
            d.get_frame_output(b_key[i])
            before.append(d)
        ctx.sync()
        t0 = time.perf_counter()
        levels = [before[i].lf_search(frames[i], originals[i], 0, 63)[0] for i in range(count)]
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        del decs, before
        return wall, levels

    out = {"config": args.config, "frames": n, "macroblocks_per_frame": (pw // 16) * (ph // 16), "levels_per_round": args.levels or 4, "runs": [], "baseline": []}
    ctx.profile(True)
    batched(n)                                           # warm-up: pools, pinned tables, code objects
    for rep in range(args.reps):
        timing, levels, evaluated = batched(n)
        timing["levels"] = dict(collections.Counter(levels)); timing["evaluated_mean"] = float(np.mean(evaluated)); timing["evaluated_max"] = int(max(evaluated))
        out["runs"].append(timing)
        print("lf_search_probe: %d frames, repetition %d: call %.1f ms in %d rounds: reconstruct %.1f, candidates %.1f (%.0f GB/s), filter %.1f, score %.1f, choose %.1f, finish %.1f; "
              "levels %s" % (n, rep, timing["call_ms"], timing["rounds"], timing["reconstruct_ms"], timing["candidates_ms"], timing["candidates_bytes_per_s"] / 1e9, timing["filter_ms"],
                             timing["score_ms"], timing["choose_ms"], timing["finish_ms"], timing["levels"]), flush=True)
    if args.baseline:
        m = min(args.baseline, n)
        looped(min(2, m)); batched(m)                    # warm-up of both on the small size
        for rep in range(args.reps):
            loop_ms, loop_levels = looped(m)
            timing, levels, _ = batched(m)
            out["baseline"].append({"frames": m, "loop_ms": loop_ms, "batched_ms": timing["python_call_ms"], "batched": timing, "levels_equal": loop_levels == levels})
            print("lf_search_probe: %d frames, repetition %d: the loop of aa_stream_lf_search %.1f ms, the batched call %.1f ms; levels %s"
                  % (m, rep, loop_ms, timing["python_call_ms"], "equal" if loop_levels == levels else "DIFFER: %s / %s" % (loop_levels, levels)), flush=True)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
