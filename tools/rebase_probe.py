"""Probe of the batched rebase (aa_rebase_batch): the first inter frame of each of the benchmark's 120 distinct 1080p streams, 4x over --
480 decoders that have decoded their key frame, each given that inter frame's records and a target made on the device (the frame as
the stream itself decodes it, plus integer noise), all in ONE call.  Reports, per call: the wall time of the C call and what
aa_rebase_last_timing says of it -- job table up + the two kernels and the download between HIP events, the records built on the host,
the frames appended --, macroblocks/s, and beside it, from the same process, the time of decode_batch of the very frames the call
appended (HIP events on the compute stream).  Every repetition rebases onto the references the previous one left (the new frames
refresh LAST), so the work is the same each time.  Before anything is printed a sample of the decoded new frames is compared with its
target (mean absolute luma error; a rebased frame comes out within the quantiser's error of it).

    python tools/rebase_probe.py [--reps 3] [--warmup 1] [--streams 120] [--copies 4] [--device] [--out results.json]

--device: afterwards, in the same process, the same frames on twin decoders through aa_rebase_device_batch (Context.rebase( records=False ):
the records compacted on the device and kept there); its figures go under "device" in the result, the download leg being the count
words alone, the host-records leg 0 and the append leg bookkeeping.

Kernel times (k_rebase_inter, k_rebase_intra, and k_recon_inter4 on the same frames -- the yardstick: the inter kernel does that
kernel's loads plus one read of the target and an 800-byte store per macroblock): a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/rebase_probe.py --reps 1 --warmup 0`.  profiles/rebase_batch.md holds what was measured."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p_inter_lf")
    ap.add_argument("--streams", type=int, default=120)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=4, help="new frames compared with their targets")
    ap.add_argument("--out", help="also write the results as JSON to this file")
    ap.add_argument("--device", action="store_true", help="then the same frames on twin decoders through aa_rebase_device_batch (records kept in HBM)")
    args = ap.parse_args()
    import torch
    import workload

    paths = workload.make_streams(args.config, 2, list(range(100, 100 + args.streams)))
    ctx = aa.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(7)
    headers, records, targets, keys, size = [], [], [], [], None
    for i, p in enumerate(paths):
        w, h, frames = aa.read_ivf(p)
        size = (w, h)
        parser = aa.Parser(w, h)
        parser.parse(frames[0])
        hdr, mb, _ = parser.parse(frames[1])
        headers.append(hdr); records.append(mb); keys.append(frames[0])
        # the target: the inter frame as the stream decodes it, plus noise in [-amp, amp]
        d = aa.Decoder(ctx, w, h)
        d.get_frame_output(frames[0])
        _, fi = d.get_frame_output(frames[1])
        pw, ph = d.padded_width, d.padded_height
        planes = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
        d.export_raster_device(fi, *[t.data_ptr() for t in planes])
        ctx.sync()
        amp = (3, 12, 40)[i % 3]
        for t in planes:
            nz = torch.randint(-amp, amp + 1, t.shape, generator=gen, device="cuda", dtype=torch.int16)
            t.copy_((t.to(torch.int16) + nz).clamp_(0, 255).to(torch.uint8))
        targets.append(tuple(planes))
        del d
    torch.cuda.synchronize()
    decs, twins = [], []
    for group in [decs] + ([twins] if args.device else []):
        for c in range(args.copies):
            for i in range(len(paths)):
                d = aa.Decoder(ctx, *size)
                d.get_frame_output(keys[i])
                group.append(d)
    ctx.sync()
    n = len(decs)
    b_hdr, b_mb, b_t = headers * args.copies, records * args.copies, targets * args.copies
    nmb = sum(m.size for m in b_mb)
    intra = sum(int((m["ref_frame"] == 0).sum()) for m in b_mb)
    compute = torch.cuda.ExternalStream(ctx.compute_stream(), device=torch.device("cuda", ctx.device))

    def measure(decs, on_device):
        runs = []
        for rep in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            results = ctx.rebase(decs, b_hdr, b_mb, b_t, records=not on_device)
            wall_py = (time.perf_counter() - t0) * 1e3
            timing = ctx.rebase_timing()
            fis = [r[0] for r in results]
            blocks = sum(r[1] if on_device else len(r[2]) for r in results)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(compute)
            ctx.decode_batch(decs, fis)
            ev[1].record(compute)
            ev[1].synchronize()
            timing["decode_batch_ms"] = ev[0].elapsed_time(ev[1])
            timing["python_call_ms"] = wall_py
            timing["coeff_blocks"] = blocks
            if rep == args.warmup + args.reps - 1:
                for k in np.linspace(0, n - 1, args.sample).astype(int):
                    y = decs[k].raster(fis[k])[0].astype(np.int32)
                    err = np.abs(y - b_t[k][0].cpu().numpy().astype(np.int32)).mean()
                    timing.setdefault("sample_mean_abs_luma_error", []).append(round(float(err), 3))
                    if err > 8:
                        print("rebase_probe: WARNING: decoder %d's new frame is %.2f grey levels from its target on average" % (k, err), file=sys.stderr)
            for d, fi in zip(decs, fis):
                d.release_before(fi)
            del results
            if rep >= args.warmup:
                runs.append(timing)
        mean = {k: float(np.mean([r[k] for r in runs])) for k in ("call_ms", "kernels_ms", "download_ms", "records_ms", "append_ms", "decode_batch_ms", "python_call_ms")}
        out = {"config": args.config, "frames": n, "macroblocks": nmb, "intra_macroblocks": intra, "reps": args.reps, "runs": runs, "mean": mean,
               "macroblocks_per_s_call": nmb / mean["call_ms"] * 1e3, "macroblocks_per_s_kernels": nmb / mean["kernels_ms"] * 1e3,
               "share_download": mean["download_ms"] / mean["call_ms"], "share_host_records": mean["records_ms"] / mean["call_ms"],
               "share_append": mean["append_ms"] / mean["call_ms"]}
        print("rebase%s of %d frames (%d macroblocks, %d intra): call %.1f ms = up + kernels %.1f, download %.1f, host records %.1f, append %.1f; %.1f M macroblocks/s; decode_batch of the same frames %.1f ms"
              % (", records kept on the device," if on_device else "", n, nmb, intra, mean["call_ms"], mean["kernels_ms"], mean["download_ms"], mean["records_ms"], mean["append_ms"],
                 out["macroblocks_per_s_call"] / 1e6, mean["decode_batch_ms"]), flush=True)
        return out

    out = measure(decs, False)
    if args.device:
        out["device"] = measure(twins, True)
        out["device"]["coeff_blocks_equal_host_path"] = out["device"]["runs"][-1]["coeff_blocks"] == out["runs"][-1]["coeff_blocks"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
