"""Probe of the batched frame-size estimate and target-size quantiser search (aa_estimate_size_batch, aa_target_size_batch): the benchmark's
distinct 1080p streams, several times over -- 480 decoders, each given the stream's first picture (KEY kind, no state needed) and, once
that is decoded, the stream's second picture (INTER kind), one call per kind and quality.  Per kind and quality it reports
  - one estimate round at the stream's own quantiser index (Context.estimate_frame_sizes),
  - a whole search (Context.target_size_q over aa.target_size_range()) for a target of half that estimate, with the rounds it took,
  - the same pictures' encode at the chosen indices through aa_encode_device_batch (Context.encode_frames( records=False )), from the
    same session: the encode the search chooses the quantiser FOR, and the yardstick of what a round costs,
each as the wall time of the C call and the legs aa_target_size_last_timing / aa_encode_last_timing give; and (--reference) the seconds
oracle/_ref/xc-enc -F takes on one core of the same host for ONE stream's two pictures at the same targets: the one-picture file gives
the key frame's, the two-picture file minus that the inter frame's (search and final encode together, processes timed whole).

    python tools/target_size_probe.py [--streams 120] [--copies 4] [--reference] [--out results.json]

Every timed call follows one untimed call of its kind (the estimate over the same jobs, the encode over four more decoders), so that no
first launch and no first piece of the pool is inside a figure.  Run it in five fresh processes and take medians; profiles/target_size_batch.md holds what was measured."""
import argparse
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


def reference_seconds(w, h, pictures, targets, quality):
    """oracle/_ref/xc-enc -F over `pictures` (display planes, one or two) on one core -> seconds, or None."""
    enc = os.path.join(ROOT, "oracle", "_ref", "xc-enc")
    if not os.path.exists(enc):
        return None
    with tempfile.TemporaryDirectory() as td:
        src, out, sizes = os.path.join(td, "in.y4m"), os.path.join(td, "out.ivf"), os.path.join(td, "sizes.txt")
        with open(src, "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h))
            for planes in pictures:
                f.write(b"FRAME\n")
                for p in planes:
                    f.write(np.ascontiguousarray(p).tobytes())
        with open(sizes, "w") as f:
            f.write("".join("%d\n" % t for t in targets[:len(pictures)]))
        t0 = time.perf_counter()
        subprocess.run(["taskset", "-c", str(sorted(os.sched_getaffinity(0))[0]), enc, "-i", "y4m", "-F", sizes, "-q", quality, "-o", out, src],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p_inter_lf")
    ap.add_argument("--streams", type=int, default=120)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--reference", action="store_true", help="also time oracle/_ref/xc-enc -F on one stream's two pictures")
    ap.add_argument("--out", help="also write the results as JSON to this file")
    args = ap.parse_args()
    import torch
    import workload

    paths = workload.make_streams(args.config, 2, list(range(100, 100 + args.streams)))
    ctx = aa.Context(0)
    headers, targets, frames0, size, display = [[], []], [[], []], [], None, None
    for i, p in enumerate(paths):
        w, h, frames = aa.read_ivf(p)
        size = (w, h)
        parser = aa.Parser(w, h)
        d = aa.Decoder(ctx, w, h)
        frames0.append(frames[0])
        for k in (0, 1):
            hdr, _, _ = parser.parse(frames[k])
            if hdr["segmentation_enabled"]:
                raise SystemExit("target_size_probe: %s uses segmentation" % p)
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
    out = {"config": args.config, "pictures_per_kind": n, "macroblocks_per_kind": nmb, "qualities": {}}

    for quality in ("best", "rt"):
        decs = [aa.Decoder(ctx, *size) for _ in range(n)]
        q = {}
        lo, hi = aa.target_size_range()
        for k, kind in enumerate(("key", "inter")):
            if k == 1:                     # the inter kind predicts from the stream's own first frame
                for d, data in zip(decs, frames0 * args.copies):
                    d.parse_and_decode_frame(data)
                ctx.sync()
            own_q = [hh["q_index"] for hh in b_hdr[k]]
            carry = (0, 0, 0, 0)           # the stream's first inter frame: vector cost tables not filled yet
            ctx.estimate_frame_sizes(decs, b_t[k], own_q, key_frame=(k == 0), quality=quality, carry=carry)      # untimed: the kind's first launches, the pool's first pieces
            t0 = time.perf_counter()
            est = ctx.estimate_frame_sizes(decs, b_t[k], own_q, key_frame=(k == 0), quality=quality, carry=carry)
            round_wall = (time.perf_counter() - t0) * 1e3
            round_t = ctx.target_size_timing()
            goals = [max(1, e[0] // 2) for e in est]
            t0 = time.perf_counter()
            res = ctx.target_size_q(decs, b_t[k], goals, lo, hi, key_frame=(k == 0), quality=quality, carry=carry)
            search_wall = (time.perf_counter() - t0) * 1e3
            search_t = ctx.target_size_timing()
            chosen = [r[0] for r in res]
            # the encode the search is for, on twins so that the estimate's decoders stay where they are
            twins = [aa.Decoder(ctx, *size) for _ in range(n + 4)]
            if k == 1:
                for d, data in zip(twins, frames0 * args.copies + frames0[:4]):
                    d.parse_and_decode_frame(data)
                ctx.sync()
            hdrs = [dict(hh, q_index=c, quant=[aa.quant_factors(c)] * 4) for hh, c in zip(b_hdr[k], chosen)]
            ctx.encode_frames(twins[n:], hdrs[:4], b_t[k][:4], quality=quality, records=False)                  # untimed: the kind's first launch
            twins = twins[:n]
            t0 = time.perf_counter()
            ctx.encode_frames(twins, hdrs, b_t[k], quality=quality, records=False)
            encode_wall = (time.perf_counter() - t0) * 1e3
            encode_t = ctx.encode_timing()
            del twins
            q[kind] = {"estimate_round": dict(round_t, python_call_ms=round_wall), "search": dict(search_t, python_call_ms=search_wall),
                       "encode_device": dict(encode_t, python_call_ms=encode_wall), "estimates_per_search": float(np.mean([len(r[1]) for r in res])),
                       "chosen_q": {"min": int(min(chosen)), "median": float(np.median(chosen)), "max": int(max(chosen))},
                       "estimate_at_own_q": {"min": int(min(e[0] for e in est)), "median": float(np.median([e[0] for e in est])), "max": int(max(e[0] for e in est))}}
            if args.reference:
                goal = [goals[0], goals[0]]
                one = reference_seconds(size[0], size[1], display[:1], goal, quality)
                two = reference_seconds(size[0], size[1], display, goal, quality) if k == 1 else None
                if one and (k == 0 or two):
                    q[kind]["reference_s_per_frame_one_core"] = one if k == 0 else two - one
            ref = q[kind].get("reference_s_per_frame_one_core")
            print("target size -q %s, %s: %d pictures: one estimate round %.1f ms (decisions %.1f, tokens %.1f, down %.1f, host %.1f); search %.1f ms in %d rounds "
                  "(decisions %.1f, tokens %.1f, down %.1f, host %.1f), %.2f estimates a picture, q %s; the encode at the chosen q, records kept on the device: %.1f ms%s"
                  % (quality, kind, n, round_t["call_ms"], round_t["decisions_ms"], round_t["tokens_ms"], round_t["download_ms"], round_t["host_ms"], search_t["call_ms"],
                     int(search_t["rounds"]), search_t["decisions_ms"], search_t["tokens_ms"], search_t["download_ms"], search_t["host_ms"], q[kind]["estimates_per_search"],
                     q[kind]["chosen_q"], encode_t["call_ms"], "; xc-enc -F on one core: %.2f s a frame" % ref if ref else ""), flush=True)
        out["qualities"][quality] = q
        del decs
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
