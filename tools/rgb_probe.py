"""Bandwidth probe of the RGB conversion (aa_render_rgb_async): the first frame of each of the benchmark's 120 distinct 1080p streams,
decoded once and rendered 4x over into one batch of 480 frames, in every format.  Times the render call between HIP events on
torch's current stream (the call orders itself on it) and reports ms per batch and effective GB/s = (bytes read + bytes written) /
time, reads counted as the display rectangle's Y, U and V bytes.  One frame per format is checked against tests/rgb_reference.py.

    python tools/rgb_probe.py [--reps 20] [--warmup 3] [--out results.json]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/rgb_probe.py --reps 3` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import alfalfa_amd as aa  # noqa: E402

BYTES_OUT = {"rgb24": 3, "rgba": 4, "chw_u8": 3, "chw_f16": 6, "chw_bf16": 6, "chw_f32": 12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p_inter_lf")
    ap.add_argument("--streams", type=int, default=120)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--formats", default=",".join(BYTES_OUT))
    ap.add_argument("--out", help="also write the results as JSON to this file")
    args = ap.parse_args()
    import torch
    import workload
    import rgb_reference as rr

    paths = workload.make_streams(args.config, 1, list(range(100, 100 + args.streams)))
    ctx = aa.Context(0)
    decs, fis = [], []
    for p in paths:
        w, h, frames = aa.read_ivf(p)
        d = aa.Decoder(ctx, w, h)
        shown, fi = d.get_frame_output(frames[0])
        assert shown
        decs.append(d); fis.append(fi)
    ctx.sync()
    batch_d, batch_f = decs * args.copies, fis * args.copies
    n = len(batch_d)
    w, h = decs[0].width, decs[0].height
    bytes_in = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    results = {"config": args.config, "frames": n, "width": w, "height": h, "reps": args.reps, "formats": {}}
    for fmt in args.formats.split(","):
        out = ctx.to_rgb(batch_d, batch_f, format=fmt)
        for _ in range(args.warmup):
            ctx.to_rgb(batch_d, batch_f, format=fmt, out=out)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(args.reps):
            ctx.to_rgb(batch_d, batch_f, format=fmt, out=out)
        ev[1].record()
        ev[1].synchronize()
        ms = ev[0].elapsed_time(ev[1]) / args.reps
        k = n // 2 + 1
        got = out[k].cpu()
        got = got.view(torch.int16).numpy().view(np.uint16) if got.dtype == torch.bfloat16 else rr.as_bits(got.numpy())
        exact = bool(np.array_equal(got, rr.expected(batch_d[k].raster(batch_f[k]), w, h, fmt)))
        total = n * (bytes_in + w * h * BYTES_OUT[fmt])
        results["formats"][fmt] = {"ms_per_batch": round(ms, 4), "effective_GBps": round(total / ms / 1e6, 1), "bytes_per_batch": total, "exact": exact}
        print("%-9s %8.3f ms / %d frames  %7.1f GB/s  exact=%s" % (fmt, ms, n, total / ms / 1e6, exact), flush=True)
        del out
        torch.cuda.empty_cache()
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    if not all(r["exact"] for r in results["formats"].values()):
        raise SystemExit("rgb_probe: output differs from the restatement")


if __name__ == "__main__":
    main()
