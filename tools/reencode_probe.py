"""Probe of the batched re-encode (aa_reencode_batch): the benchmark's distinct 1080p streams, 4x over -- 480 decoders that have decoded
their key frame, each asked to encode the stream's NEXT picture (as the stream itself decodes it, made on the device) as an inter frame
predicted from that key frame, all in ONE call, in both qualities.  Reports, per quality: the wall time of the C call and what
aa_reencode_last_timing says of it -- job table and rate models up + the kernel, and the download, between HIP events; the records
built on the host; the frames appended --, macroblocks/s, the classes the decision produced, and (--reference) the time
oracle/_ref/xc-enc -r takes for ONE such frame on one core of the same host: the same two pictures written out as y4m, chunk 0 and
the prediction key frame encoded by the reference, then `xc-enc -r -W -q <quality>` over a one-frame chunk, timed as a process (its
start-up and its reading of the inputs included: tens of milliseconds beside seconds).  The reference is the yardstick.

    python tools/reencode_probe.py [--streams 120] [--copies 4] [--reps 1] [--warmup 0] [--reference] [--device] [--out results.json]

--device: per quality, in the same process, the same frames on fresh decoders through aa_reencode_device_batch
(Context.reencode_as_inter( records=False ): the records compacted on the device and kept there); its figures go under "device" in the
quality's result, the download leg being the count and row words alone, the host-records leg 0 and the append leg bookkeeping.

Before anything is printed a sample of the decoded new frames is compared with its target (mean absolute luma error).
profiles/reencode_batch.md and profiles/reencode_device.md hold what was measured."""
import argparse
import collections
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import alfalfa_amd as aa  # noqa: E402

MODES = ("intra DC", "intra V", "intra H", "intra TM", "B_PRED", "NEARESTMV", "NEARMV", "ZEROMV", "NEWMV", "SPLITMV")


def reference_seconds(w, h, first, second, q_index, quality):
    """oracle/_ref/xc-enc -r over the one-frame chunk `second` after the one-frame chunk `first` (display planes) -> seconds, or None."""
    ref = os.path.join(ROOT, "oracle", "_ref")
    enc, state_tool = os.path.join(ref, "xc-enc"), os.path.join(ref, "ref_state")
    if not (os.path.exists(enc) and os.path.exists(state_tool)):
        return None

    def y4m(path, planes):
        with open(path, "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\nFRAME\n" % (w, h))
            for p in planes:
                f.write(np.ascontiguousarray(p).tobytes())

    with tempfile.TemporaryDirectory() as td:
        c0y, c1y, c0i, pred, state, out = (os.path.join(td, f) for f in ("c0.y4m", "c1.y4m", "c0.ivf", "pred.ivf", "c0.state", "out.ivf"))
        y4m(c0y, first); y4m(c1y, second)
        quiet = dict(check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        subprocess.run([enc, "-i", "y4m", "-y", str(q_index), "-q", quality, "-o", c0i, c0y], **quiet)
        subprocess.run([enc, "-i", "y4m", "-y", str(q_index), "-q", quality, "-o", pred, c1y], **quiet)
        subprocess.run([state_tool, "save", c0i, "1", state], **quiet)
        t0 = time.perf_counter()
        subprocess.run(["taskset", "-c", str(sorted(os.sched_getaffinity(0))[0]), enc, "-r", "-W", "-q", quality, "-i", "y4m", "-p", pred, "-I", state, "-o", out, c1y], **quiet)
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p_inter_lf")
    ap.add_argument("--streams", type=int, default=120)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=0)
    ap.add_argument("--sample", type=int, default=4, help="new frames compared with their targets")
    ap.add_argument("--reference", action="store_true", help="also time oracle/_ref/xc-enc -r on one such frame")
    ap.add_argument("--out", help="also write the results as JSON to this file")
    ap.add_argument("--device", action="store_true", help="then, per quality, the same frames on fresh decoders through aa_reencode_device_batch (records kept in HBM)")
    args = ap.parse_args()
    import torch
    import workload

    paths = workload.make_streams(args.config, 2, list(range(100, 100 + args.streams)))
    ctx = aa.Context(0)
    headers, targets, keys, size, display = [], [], [], None, None
    for i, p in enumerate(paths):
        w, h, frames = aa.read_ivf(p)
        size = (w, h)
        parser = aa.Parser(w, h)
        parser.parse(frames[0])
        hdr, _, _ = parser.parse(frames[1])
        if hdr["segmentation_enabled"]:
            raise SystemExit("reencode_probe: %s uses segmentation" % p)
        headers.append(hdr); keys.append(frames[0])
        d = aa.Decoder(ctx, w, h)
        d.get_frame_output(frames[0])
        _, fi = d.get_frame_output(frames[1])
        pw, ph = d.padded_width, d.padded_height
        planes = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
        d.export_raster_device(fi, *[t.data_ptr() for t in planes])
        ctx.sync()
        targets.append(tuple(planes))
        if i == 0:
            cw, ch = (w + 1) // 2, (h + 1) // 2
            display = [[pl[:hh, :ww] for pl, (hh, ww) in zip(d.raster(k), ((h, w), (ch, cw), (ch, cw)))] for k in (0, fi)]
        del d
    torch.cuda.synchronize()
    n = len(paths) * args.copies
    b_hdr, b_t = headers * args.copies, targets * args.copies
    nmb = sum(hh["num_macroblocks"] for hh in b_hdr)
    out = {"config": args.config, "frames": n, "macroblocks": nmb, "reps": args.reps, "qualities": {}}

    def measure(quality, on_device):
        runs, classes = [], collections.Counter()
        for rep in range(args.warmup + args.reps):
            decs = []
            for c in range(args.copies):
                for i in range(len(paths)):
                    d = aa.Decoder(ctx, *size)
                    d.get_frame_output(keys[i])
                    decs.append(d)
            ctx.sync()
            t0 = time.perf_counter()
            results = ctx.reencode_as_inter(decs, b_hdr, b_t, quality=quality, records=not on_device)
            wall_py = (time.perf_counter() - t0) * 1e3
            timing = ctx.reencode_timing()
            timing["python_call_ms"] = wall_py
            timing["coeff_blocks"] = sum(r[1] if on_device else len(r[2]) for r in results)
            fis = [r[0] for r in results]
            ctx.decode_batch(decs, fis)
            if rep == args.warmup + args.reps - 1:
                for d, r in zip(decs[:len(paths)], results[:len(paths)]):
                    ym, cnt = np.unique(d.read_records(r[0])[1]["y_mode"] if on_device else r[1]["y_mode"], return_counts=True)
                    for m, k in zip(ym, cnt):
                        classes[MODES[m]] += int(k) * args.copies
                for k in np.linspace(0, n - 1, args.sample).astype(int):
                    y = decs[k].raster(fis[k])[0].astype(np.int32)
                    err = np.abs(y - b_t[k][0].cpu().numpy().astype(np.int32)).mean()
                    timing.setdefault("sample_mean_abs_luma_error", []).append(round(float(err), 3))
                    if err > 8:
                        print("reencode_probe: WARNING: decoder %d's new frame is %.2f grey levels from its target on average" % (k, err), file=sys.stderr)
            del results, decs
            if rep >= args.warmup:
                runs.append(timing)
            print("reencode_probe: -q %s%s, repetition %d: call %.1f ms" % (quality, ", records kept on the device" if on_device else "", rep, timing["call_ms"]), file=sys.stderr, flush=True)
        mean = {k: float(np.mean([r[k] for r in runs])) for k in ("call_ms", "kernels_ms", "download_ms", "records_ms", "append_ms", "python_call_ms")}
        q = {"runs": runs, "mean": mean, "classes": dict(classes), "macroblocks_per_s_call": nmb / mean["call_ms"] * 1e3,
             "frames_per_s_call": n / mean["call_ms"] * 1e3, "ms_per_frame": mean["call_ms"] / n, "share_kernel": mean["kernels_ms"] / mean["call_ms"]}
        if args.reference and not on_device:
            s = reference_seconds(size[0], size[1], display[0], display[1], headers[0]["q_index"], quality)
            q["reference_s_per_frame_one_core"] = s
            if s:
                q["reference_frames_per_s_one_core"] = 1.0 / s
        print("re-encode -q %s%s of %d frames (%d macroblocks): call %.1f ms = up + kernel%s %.1f, download %.1f, host records %.1f, append %.1f; %.2f ms a frame, %.0f frames/s%s; %s"
              % (quality, ", records kept on the device," if on_device else "", n, nmb, mean["call_ms"], "s" if on_device else "", mean["kernels_ms"], mean["download_ms"],
                 mean["records_ms"], mean["append_ms"], q["ms_per_frame"], q["frames_per_s_call"],
                 "; xc-enc -r on one core: %.2f s a frame" % q["reference_s_per_frame_one_core"] if q.get("reference_s_per_frame_one_core") else "", dict(classes)), flush=True)
        return q

    for quality in ("best", "rt"):
        out["qualities"][quality] = measure(quality, False)
        if args.device:
            q = out["qualities"][quality]["device"] = measure(quality, True)
            q["coeff_blocks_equal_host_path"] = q["runs"][-1]["coeff_blocks"] == out["qualities"][quality]["runs"][-1]["coeff_blocks"]
            q["classes_equal_host_path"] = q["classes"] == out["qualities"][quality]["classes"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
