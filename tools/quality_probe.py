"""Probe of the batched quality measure (aa_quality_batch_async): the first frame of each of the benchmark's 120 distinct 1080p streams,
decoded once and scored 4x over in one batch of 480 frames against originals made on the device (the decoded planes plus integer
noise), with planes="y" and planes="yuv".  Times the call between HIP events on torch's current stream (the call orders itself on it)
and reports ms per batch and GB/s = both planes' bytes read / time.  Before anything is printed, a sample of frames is checked
against aa_ssim_host (SSIM, bit for bit) and numpy (squared error).

For comparison it also times the only route to the same numbers without this call: aa_stream_download of each frame plus aa_ssim_host
per plane, on the wall clock (--host-frames of the distinct frames; the batch figure is that time scaled to the batch).

    python tools/quality_probe.py [--reps 20] [--warmup 3] [--host-frames 120] [--out results.json]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/quality_probe.py --reps 3` in a run of its own."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import alfalfa_amd as aa  # noqa: E402
from alfalfa_amd import capi  # noqa: E402


def ssim_host(a, b):
    out = C.c_double()
    capi.check(capi.lib().aa_ssim_host(a.tobytes(), b.tobytes(), a.shape[1], a.shape[0], C.byref(out)))
    return out.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p_inter_lf")
    ap.add_argument("--streams", type=int, default=120)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=6, help="frames checked against aa_ssim_host and numpy")
    ap.add_argument("--host-frames", type=int, default=120, help="frames timed on the download + aa_ssim_host route (0: skip)")
    ap.add_argument("--out", help="also write the results as JSON to this file")
    args = ap.parse_args()
    import torch
    import workload

    paths = workload.make_streams(args.config, 1, list(range(100, 100 + args.streams)))
    ctx = aa.Context(0)
    decs, fis = [], []
    for p in paths:
        w, h, frames = aa.read_ivf(p)
        d = aa.Decoder(ctx, w, h)
        shown, fi = d.get_frame_output(frames[0])
        assert shown
        decs.append(d); fis.append(fi)
    pw, ph = decs[0].padded_width, decs[0].padded_height
    # originals: the decoded planes plus noise in [-amp, amp], made on the device
    gen = torch.Generator(device="cuda").manual_seed(7)
    origs = []
    for i, (d, fi) in enumerate(zip(decs, fis)):
        planes = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
        d.export_raster_device(fi, *[t.data_ptr() for t in planes])
        origs.append(planes)
    ctx.sync()
    for i, planes in enumerate(origs):
        amp = (3, 12, 40)[i % 3]
        for t in planes:
            nz = torch.randint(-amp, amp + 1, t.shape, generator=gen, device="cuda", dtype=torch.int16)
            t.copy_((t.to(torch.int16) + nz).clamp_(0, 255).to(torch.uint8))
    torch.cuda.synchronize()
    batch_d, batch_f, batch_o = decs * args.copies, fis * args.copies, [tuple(o) for o in origs] * args.copies
    n = len(batch_d)
    plane_bytes = [pw * ph, pw * ph // 4, pw * ph // 4]
    results = {"config": args.config, "frames": n, "padded_width": pw, "padded_height": ph, "reps": args.reps, "planes": {}}
    lines = []
    for planes in ("y", "yuv"):
        np_ = len(planes)
        q = ctx.quality(batch_d, batch_f, batch_o, planes=planes)
        out = (q.ssim, q.sse)
        for _ in range(args.warmup):
            ctx.quality(batch_d, batch_f, batch_o, planes=planes, out=out)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(args.reps):
            ctx.quality(batch_d, batch_f, batch_o, planes=planes, out=out)
        ev[1].record()
        ev[1].synchronize()
        ms = ev[0].elapsed_time(ev[1]) / args.reps
        ssim, sse = q.ssim.cpu().numpy(), q.sse.cpu().numpy()
        exact = True
        for k in np.linspace(0, n - 1, args.sample).astype(int):
            raster = batch_d[k].raster(batch_f[k])
            for p in range(np_):
                b = batch_o[k][p].cpu().numpy()
                diff = raster[p].astype(np.int64) - b.astype(np.int64)
                exact = exact and ssim[k, p] == ssim_host(raster[p], b) and int(sse[k, p]) == int((diff * diff).sum())
        total = 2 * n * sum(plane_bytes[:np_])
        results["planes"][planes] = {"ms_per_batch": round(ms, 4), "GBps_read": round(total / ms / 1e6, 1), "bytes_read_per_batch": total,
                                     "fraction_of_6.3TBps": round(total / ms / 1e6 / 6300.0, 3), "exact": bool(exact),
                                     "mean_ssim": float(ssim.mean())}
        lines.append("%-4s %8.3f ms / %d frames  %7.1f GB/s read  exact=%s" % (planes, ms, n, total / ms / 1e6, exact))
    if not all(r["exact"] for r in results["planes"].values()):
        raise SystemExit("quality_probe: values differ from aa_ssim_host / numpy")
    print("\n".join(lines), flush=True)
    if args.host_frames > 0:
        # the route without the batched call: every frame downloaded, every plane scored by one core
        k = min(args.host_frames, len(decs))
        host_orig = [[t.cpu().numpy() for t in o] for o in origs[:k]]
        for planes in ("y", "yuv"):
            np_ = len(planes)
            t0 = time.perf_counter()
            t_dl = 0.0
            for i in range(k):
                t1 = time.perf_counter()
                raster = decs[i].raster(fis[i])
                t_dl += time.perf_counter() - t1
                for p in range(np_):
                    ssim_host(raster[p], host_orig[i][p])
            dt = time.perf_counter() - t0
            r = {"frames_timed": k, "ms_per_frame": round(dt / k * 1e3, 3), "download_ms_per_frame": round(t_dl / k * 1e3, 3),
                 "ms_per_batch_scaled": round(dt / k * n * 1e3, 1)}
            results["planes"][planes]["host_route"] = r
            print("%-4s host route: %.3f ms / frame (download %.3f) -> %.1f ms / %d frames" % (planes, r["ms_per_frame"], r["download_ms_per_frame"],
                                                                                                r["ms_per_batch_scaled"], n), flush=True)
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
