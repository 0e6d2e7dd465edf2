"""Probe of the batched hashes (aa_hash_decoders_async + aa_ctx_hash_wait) against the per-stream route they stand beside: the first
frame of each of the benchmark's 120 distinct 1080p streams, decoded by `copies` decoders each -- 480 decoders, each with its own
raster, as at a chunk boundary of the pipelined decode.

  batch        one cold Context.decoder_hashes over all of them: wall time around call + wait, and the kernel's time between two HIP
               events on the hash stream (the compute stream is idle: the kernel starts at once).  From it: bytes walked per second per
               chain, and cycles per byte at the device's clock against the 7-instruction loop.
  per stream   the parent route on decoders of the same streams whose caches are cold: Decoder.decoder_hash one by one (stream sync,
               blocking download of the raster, chain on one host core); `--host` of them are timed and the figure scaled to the batch.
  break-even   batches of 1, 2, 4, ... fresh decoders both ways: the count below which the per-stream route is the faster one.

    python tools/hash_probe.py [--copies 4] [--host 16] [--out results.json]

Every value of the batch is checked against the per-stream route's for the same stream."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import alfalfa_amd as aa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p_inter_lf")
    ap.add_argument("--streams", type=int, default=120)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--host", type=int, default=16, help="decoders timed on the per-stream route")
    ap.add_argument("--out", help="also write the results as JSON to this file")
    args = ap.parse_args()
    import torch
    import workload

    paths = workload.make_streams(args.config, 1, list(range(100, 100 + args.streams)))
    first = [aa.read_ivf(p) for p in paths]
    ctx = aa.Context(0)
    device = torch.device("cuda", ctx.device)

    def fresh(k):
        """k decoders, decoder i on the key frame of stream i % streams, decoded in batches; caches cold"""
        ds = [aa.Decoder(ctx, first[i % len(first)][0], first[i % len(first)][1]) for i in range(k)]
        for lo in range(0, k, 240):
            part = ds[lo:lo + 240]
            ctx.decode_batch(part, ctx.submit_frames([(d, first[(lo + j) % len(first)][2][0]) for j, d in enumerate(part)], route="host"))
        ctx.sync()
        return ds

    def batch_ms(ds):
        hs = torch.cuda.ExternalStream(ctx.hash_stream(), device=device)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t0 = time.perf_counter()
        ev[0].record(hs)
        pending = ctx.decoder_hashes(ds, wait=False)
        ev[1].record(hs)
        got = pending.result()
        wall = (time.perf_counter() - t0) * 1e3
        ev[1].synchronize()
        return got, wall, ev[0].elapsed_time(ev[1])

    def host_ms(ds):
        t0 = time.perf_counter()
        got = [d.decoder_hash() for d in ds]
        return got, (time.perf_counter() - t0) * 1e3

    n = len(first) * args.copies
    w, h = first[0][0], first[0][1]
    info = ctx.info()
    batch_ms(fresh(1))                                   # (the hash stream, its first buffer and the code object are in place)
    ctx.hash_stats(reset=True)
    decs = fresh(n)
    got, wall, kernel = batch_ms(decs)
    st = ctx.hash_stats()
    twins = fresh(args.host)
    want, host = host_ms(twins)
    assert got[:args.host] == want, "hash_probe: the batch differs from the per-stream route"
    assert all(got[i] == got[i % len(first)] for i in range(n))
    per_chain = st["bytes"] / st["chains"]
    clock = info["clock_mhz"] or 2400
    res = {"config": args.config, "decoders": n, "width": w, "height": h, "chains": st["chains"], "bytes_walked": st["bytes"],
           "batch_wall_ms": round(wall, 3), "batch_kernel_ms": round(kernel, 3),
           "chain_MBps": round(per_chain / kernel / 1e3, 2), "clock_mhz": clock, "cycles_per_byte": round(kernel * 1e-3 * clock * 1e6 / per_chain, 2),
           "host_decoders_timed": args.host, "host_ms_per_decoder": round(host / args.host, 3), "host_ms_scaled": round(host / args.host * n, 1),
           "speedup_wall": round(host / args.host * n / wall, 2), "break_even": []}
    print("batch      %4d decoders  %9.3f ms wall  %9.3f ms kernel  %d chains  %.2f MB/s per chain  %.2f cycles/byte at %d MHz"
          % (n, wall, kernel, st["chains"], res["chain_MBps"], res["cycles_per_byte"], clock), flush=True)
    print("per stream %4d decoders  %9.3f ms each  -> %.1f ms for %d  (batch %.2fx)" % (args.host, host / args.host, res["host_ms_scaled"], n, res["speedup_wall"]), flush=True)
    del decs, twins
    k = 1
    while k <= min(n, 64):
        _, bw, bk = batch_ms(fresh(k))
        _, hm = host_ms(fresh(k))
        res["break_even"].append({"decoders": k, "batch_wall_ms": round(bw, 3), "batch_kernel_ms": round(bk, 3), "per_stream_ms": round(hm, 3)})
        print("%3d decoders: batch %8.3f ms wall (%8.3f kernel), per stream %8.3f ms" % (k, bw, bk, hm), flush=True)
        k *= 2
    faster = [e["decoders"] for e in res["break_even"] if e["batch_wall_ms"] < e["per_stream_ms"]]
    res["batch_faster_from"] = min(faster) if faster else None
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
