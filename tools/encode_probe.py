"""Probe of the batched forward encoder (aa_encode_batch): the benchmark's distinct 1080p streams, several times over -- 480 fresh decoders,
each asked to encode the stream's first picture as a KEY frame and then, once that is decoded, the stream's second picture as an INTER
frame predicted from it (the pictures are the stream's own decoded frames, made on the device), each kind in ONE call, in both qualities.
Reports, per quality and kind: the wall time of the C call and what aa_encode_last_timing says of it -- job table and cost blocks up +
the kernel, and the download, between HIP events; the records built on the host; the frames appended --, macroblocks/s, the classes the
decision produced, and (--reference) the time oracle/_ref/xc-enc -i y4m -y QI -q <quality> takes on one core of the same host for the
same two pictures of ONE stream: the one-picture file gives the key frame's seconds, the two-picture file minus that the inter frame's
(processes timed whole: start-up and the reading of the input included, tens of milliseconds beside seconds).  The parent of this call is
the reference's encoder; it is the yardstick.

    python tools/encode_probe.py [--streams 120] [--copies 4] [--reps 1] [--warmup 0] [--reference] [--device] [--two-pass] [--out results.json]

--two-pass: per quality, in the same process, the same KEY pictures on fresh decoders through aa_encode_two_pass_batch (Context.encode_frames(
two_pass=True ): the reference's second pass with trellis quantisation behind the first); its figures go under "two_pass", beside them the
ratio of its call to the single-pass key call of the same process.  profiles/encode_two_pass.md holds what was measured.

--device: per quality, in the same process, the same frames on fresh decoders through aa_encode_device_batch (Context.encode_frames(
records=False ): the records compacted on the device and kept there); its figures go under "device", the download leg being the count
and row words alone, the host-records leg 0 and the append leg bookkeeping.

Before anything is printed a sample of the decoded new frames is compared with its target (mean absolute luma error).
profiles/encode_batch.md holds what was measured."""
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
LEGS = ("call_ms", "kernels_ms", "download_ms", "records_ms", "append_ms", "python_call_ms")


def reference_seconds(w, h, pictures, q_index, quality):
    """oracle/_ref/xc-enc over `pictures` (display planes, one or two) on one core -> seconds, or None."""
    enc = os.path.join(ROOT, "oracle", "_ref", "xc-enc")
    if not os.path.exists(enc):
        return None
    with tempfile.TemporaryDirectory() as td:
        src, out = os.path.join(td, "in.y4m"), os.path.join(td, "out.ivf")
        with open(src, "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h))
            for planes in pictures:
                f.write(b"FRAME\n")
                for p in planes:
                    f.write(np.ascontiguousarray(p).tobytes())
        t0 = time.perf_counter()
        subprocess.run(["taskset", "-c", str(sorted(os.sched_getaffinity(0))[0]), enc, "-i", "y4m", "-y", str(q_index), "-q", quality, "-o", out, src],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p_inter_lf")
    ap.add_argument("--streams", type=int, default=120)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=0)
    ap.add_argument("--sample", type=int, default=4, help="new frames compared with their targets")
    ap.add_argument("--reference", action="store_true", help="also time oracle/_ref/xc-enc on one stream's two pictures")
    ap.add_argument("--out", help="also write the results as JSON to this file")
    ap.add_argument("--device", action="store_true", help="then, per quality, the same frames on fresh decoders through aa_encode_device_batch (records kept in HBM)")
    ap.add_argument("--two-pass", action="store_true", help="then, per quality, the same key pictures on fresh decoders through aa_encode_two_pass_batch")
    args = ap.parse_args()
    import torch
    import workload

    paths = workload.make_streams(args.config, 2, list(range(100, 100 + args.streams)))
    ctx = aa.Context(0)
    headers, targets, size, display = [[], []], [[], []], None, None
    for i, p in enumerate(paths):
        w, h, frames = aa.read_ivf(p)
        size = (w, h)
        parser = aa.Parser(w, h)
        d = aa.Decoder(ctx, w, h)
        for k in (0, 1):
            hdr, _, _ = parser.parse(frames[k])
            if hdr["segmentation_enabled"]:
                raise SystemExit("encode_probe: %s uses segmentation" % p)
            headers[k].append(hdr)
            _, fi = d.get_frame_output(frames[k])
            pw, ph = d.padded_width, d.padded_height
            planes = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
            d.export_raster_device(fi, *[t.data_ptr() for t in planes])
            ctx.sync()
            targets[k].append(tuple(planes))
        if i == 0:
            cw, ch = (w + 1) // 2, (h + 1) // 2
            display = [[pl[:hh, :ww] for pl, (hh, ww) in zip(d.raster(k), ((h, w), (ch, cw), (ch, cw)))] for k in (0, 1)]
        del d
    torch.cuda.synchronize()
    n = len(paths) * args.copies
    b_hdr, b_t = [hh * args.copies for hh in headers], [t * args.copies for t in targets]
    nmb = sum(hh["num_macroblocks"] for hh in b_hdr[0])
    out = {"config": args.config, "frames_per_kind": n, "macroblocks_per_kind": nmb, "reps": args.reps, "qualities": {}}

    def measure(quality, on_device, two_pass=False):
        kinds = ("key",) if two_pass else ("key", "inter")
        runs, classes = {kind: [] for kind in kinds}, {kind: collections.Counter() for kind in kinds}
        for rep in range(args.warmup + args.reps):
            decs = [aa.Decoder(ctx, *size) for _ in range(n)]
            ctx.sync()
            for k, kind in enumerate(kinds):
                t0 = time.perf_counter()
                results = ctx.encode_frames(decs, b_hdr[k], b_t[k], quality=quality, records=not on_device, two_pass=two_pass)
                wall_py = (time.perf_counter() - t0) * 1e3
                timing = ctx.encode_timing()
                timing["python_call_ms"] = wall_py
                timing["coeff_blocks"] = sum(r[1] if on_device else len(r[2]) for r in results)
                fis = [r[0] for r in results]
                ctx.decode_batch(decs, fis)
                if rep == args.warmup + args.reps - 1:
                    for d, r in zip(decs[:len(paths)], results[:len(paths)]):
                        ym, cnt = np.unique(d.read_records(r[0])[1]["y_mode"] if on_device else r[1]["y_mode"], return_counts=True)
                        for m, c in zip(ym, cnt):
                            classes[kind][MODES[m]] += int(c) * args.copies
                    for s in np.linspace(0, n - 1, args.sample).astype(int):
                        y = decs[s].raster(fis[s])[0].astype(np.int32)
                        err = np.abs(y - b_t[k][s][0].cpu().numpy().astype(np.int32)).mean()
                        timing.setdefault("sample_mean_abs_luma_error", []).append(round(float(err), 3))
                        if err > 8:
                            print("encode_probe: WARNING: decoder %d's new %s frame is %.2f grey levels from its target on average" % (s, kind, err), file=sys.stderr)
                del results
                if rep >= args.warmup:
                    runs[kind].append(timing)
                print("encode_probe: -q %s %s%s%s, repetition %d: call %.1f ms" % (quality, kind, ", two passes" if two_pass else "", ", records kept on the device" if on_device else "", rep, timing["call_ms"]),
                      file=sys.stderr, flush=True)
            del decs
        q = {}
        for kind in kinds:
            mean = {leg: float(np.mean([r[leg] for r in runs[kind]])) for leg in LEGS}
            q[kind] = {"runs": runs[kind], "mean": mean, "classes": dict(classes[kind]), "macroblocks_per_s_call": nmb / mean["call_ms"] * 1e3,
                       "frames_per_s_call": n / mean["call_ms"] * 1e3, "ms_per_frame": mean["call_ms"] / n, "share_kernel": mean["kernels_ms"] / mean["call_ms"]}
        if args.reference and not on_device:
            one = reference_seconds(size[0], size[1], display[:1], headers[0][0]["q_index"], quality)
            two = reference_seconds(size[0], size[1], display, headers[0][0]["q_index"], quality)
            if one and two:
                q["key"]["reference_s_per_frame_one_core"], q["inter"]["reference_s_per_frame_one_core"] = one, two - one
        for kind in kinds:
            m, ref = q[kind]["mean"], q[kind].get("reference_s_per_frame_one_core")
            print("encode -q %s, %s frames%s%s: %d frames (%d macroblocks): call %.1f ms = up + kernel%s %.1f, download %.1f, host records %.1f, append %.1f; %.2f ms a frame, %.0f frames/s%s; %s"
                  % (quality, kind, ", two passes," if two_pass else "", ", records kept on the device," if on_device else "", n, nmb, m["call_ms"], "s" if on_device else "", m["kernels_ms"], m["download_ms"],
                     m["records_ms"], m["append_ms"], q[kind]["ms_per_frame"], q[kind]["frames_per_s_call"],
                     "; xc-enc on one core: %.2f s a frame" % ref if ref else "", q[kind]["classes"]), flush=True)
        return q

    for quality in ("best", "rt"):
        out["qualities"][quality] = measure(quality, False)
        if args.device:
            dev = out["qualities"][quality]["device"] = measure(quality, True)
            for kind in ("key", "inter"):
                host = out["qualities"][quality][kind]
                dev[kind]["coeff_blocks_equal_host_path"] = dev[kind]["runs"][-1]["coeff_blocks"] == host["runs"][-1]["coeff_blocks"]
                dev[kind]["classes_equal_host_path"] = dev[kind]["classes"] == host["classes"]
        if args.two_pass:
            two = out["qualities"][quality]["two_pass"] = measure(quality, False, two_pass=True)
            two["key"]["call_ratio_to_single_pass"] = two["key"]["mean"]["call_ms"] / out["qualities"][quality]["key"]["mean"]["call_ms"]
            two["key"]["kernels_ratio_to_single_pass"] = two["key"]["mean"]["kernels_ms"] / out["qualities"][quality]["key"]["mean"]["kernels_ms"]
            if args.device:
                dev2 = out["qualities"][quality]["two_pass_device"] = measure(quality, True, two_pass=True)
                dev2["key"]["call_ratio_to_single_pass"] = dev2["key"]["mean"]["call_ms"] / out["qualities"][quality]["device"]["key"]["mean"]["call_ms"]
                dev2["key"]["coeff_blocks_equal_host_path"] = dev2["key"]["runs"][-1]["coeff_blocks"] == two["key"]["runs"][-1]["coeff_blocks"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
