"""Probe of the batched serialisation (aa_serialize_batch) behind the batched rebase: tools/rebase_probe.py's 480 x 1080p frames -- the first
inter frame of each of the benchmark's 120 distinct streams, 4x over, rebased onto noisy targets in ONE call -- and then all 480 new
frames serialised in ONE call, with the header the prediction frame had and against the tables it was coded against.  Reports, per
repetition: the rebase call's legs (aa_rebase_last_timing: this change does not touch that call, so they are the parent commit's), the
serialise call's legs (aa_serialize_last_timing: job table up + k_serialize_tokens and the partitions' way down between HIP events; the host
workers' first partitions, which run beside the kernel; assembly and copy), the bytes that crossed the bus each way, and bytes per
macroblock of the frames written; and THE SAME CHAINS ON THE HOST'S CORES: the same 480 frames written from the records the rebase
returned by aa_serialize_host (the token lanes' own statements, serialize_common.hh, and the host half's first partition), one frame per
call, on as many worker threads as the process has cores (aa_host_cpus; argument structs built beforehand, the C calls alone are timed),
and the bytes compared with the GPU's.  Before anything is printed a sample of the written frames is parsed back and compared with the records
the rebase returned.

    python tools/serialize_probe.py [--reps 3] [--warmup 1] [--streams 120] [--copies 4] [--device] [--out results.json]

--device: the rebase leg is aa_rebase_device_batch (Context.rebase( records=False )): the frames' records stay in HBM, the serialiser
copies back the 80-byte macroblock records alone, and the records the host's chains are given are read back outside the timed legs.

profiles/serialize_batch.md holds what was measured."""
import argparse
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1080p_inter_lf")
    ap.add_argument("--streams", type=int, default=120)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=4, help="written frames parsed back and compared with the rebase's records")
    ap.add_argument("--out", help="also write the results as JSON to this file")
    ap.add_argument("--device", action="store_true", help="the rebase leg through aa_rebase_device_batch: the serialiser reads records that never left HBM")
    args = ap.parse_args()
    import torch
    import workload

    paths = workload.make_streams(args.config, 2, list(range(100, 100 + args.streams)))
    ctx = aa.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(7)
    headers, exts, befores, subs, states, records, targets, keys, size = [], [], [], [], [], [], [], [], None
    for i, p in enumerate(paths):
        w, h, frames = aa.read_ivf(p)
        size = (w, h)
        parser = aa.Parser(w, h)
        parser.parse(frames[0])
        befores.append(parser.probs().copy()); states.append(parser.export_state())
        hdr, mb, _ = parser.parse(frames[1])
        ext = parser.header_ext()
        if not ext["skip_enabled"]:         # (the rebase marks macroblocks without coefficients as skipped: the header must be able to say so)
            ext.update(skip_enabled=1, prob_skip_false=128)
        headers.append(hdr); exts.append(ext); subs.append(parser.sub_modes().copy()); records.append(mb); keys.append(frames[0])
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
    decs = []
    for c in range(args.copies):
        for i in range(len(paths)):
            d = aa.Decoder(ctx, *size)
            d.get_frame_output(keys[i])
            decs.append(d)
    ctx.sync()
    n = len(decs)
    k = args.copies
    b_hdr, b_ext, b_before, b_subs, b_mb, b_t = headers * k, exts * k, befores * k, subs * k, records * k, targets * k
    nmb = sum(m.size for m in b_mb)
    ext_structs = [capi.FrameHeaderExt.from_dict(e) for e in exts]
    b_before = [np.ascontiguousarray(b, dtype=np.uint8) for b in b_before]
    capacity = 4096 + (nmb // n) * 400          # bytes per frame: half the raw size of a frame's coefficients and more than any of these takes
    runs = []
    for rep in range(args.warmup + args.reps):
        results = ctx.rebase(decs, b_hdr, b_mb, b_t, records=not args.device)
        rebase = ctx.rebase_timing()
        fis = [r[0] for r in results]
        t0 = time.perf_counter()
        frames = ctx.serialize_frames(decs, fis, b_hdr, b_ext, probs_before=b_before, sub_modes=b_subs, capacity=capacity)
        wall_py = (time.perf_counter() - t0) * 1e3
        timing = ctx.serialize_timing()
        if args.device:                     # (the host's chains below and the parse-back want the records: read back here, outside every timed leg)
            results = [(fi,) + d.read_records(fi)[1:] for d, fi in zip(decs, fis)]
        timing = {"serialize_" + key: v for key, v in timing.items()}
        timing.update({"rebase_" + key: v for key, v in rebase.items()})
        timing["serialize_python_call_ms"] = wall_py
        timing["frame_bytes"] = sum(len(f) for f in frames)
        timing["coeff_blocks"] = sum(len(r[2]) for r in results)
        # the same frames by host cores
        L = capi.lib()
        workers = max(1, L.aa_host_cpus())
        calls, keep = [], []
        for j in range(n):
            hdr = aa.Context._header_struct(b_hdr[j])
            mbs, cf = np.ascontiguousarray(results[j][1]).reshape(-1), np.ascontiguousarray(results[j][2])
            hdr.num_coeff_blocks = len(cf)
            out, nbytes = np.zeros(capacity, np.uint8), C.c_size_t()
            sm = np.ascontiguousarray(b_subs[j], dtype=np.uint8)
            keep.append((hdr, mbs, cf, out, nbytes, sm))
            calls.append((C.byref(hdr), C.byref(ext_structs[j % len(ext_structs)]), b_before[j].ctypes.data_as(C.c_void_p), mbs.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p),
                          sm.ctypes.data_as(C.c_void_p) if len(sm) else None, len(sm), out.ctypes.data_as(C.c_void_p), capacity, C.byref(nbytes)))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(workers) as pool:
            rcs = list(pool.map(lambda a: L.aa_serialize_host(*a), calls))
        timing["host_serialize_ms"] = (time.perf_counter() - t0) * 1e3
        timing["host_workers"] = workers
        t0 = time.perf_counter()
        L.aa_serialize_host(*calls[0])
        timing["host_one_frame_one_core_ms"] = (time.perf_counter() - t0) * 1e3
        if any(rcs) or any(k[3][:k[4].value].tobytes() != f for k, f in zip(keep, frames)):
            print("serialize_probe: ERROR: the host's frames are not the GPU's", file=sys.stderr)
            sys.exit(1)
        del calls, keep
        if rep == args.warmup + args.reps - 1:
            for j in np.linspace(0, n - 1, args.sample).astype(int):
                back = aa.Parser(*size)
                back.import_state(states[j % len(paths)])
                hdr2, mb2, blocks2 = back.parse(frames[j])
                if not ((mb2 == results[j][1]).all() and (blocks2 == results[j][2]).all()):
                    print("serialize_probe: ERROR: frame %d parses back to other records than the rebase returned" % j, file=sys.stderr)
                    sys.exit(1)
        ctx.decode_batch(decs, fis)
        for d, fi in zip(decs, fis):
            d.release_before(fi)
        del results, frames
        if rep >= args.warmup:
            runs.append(timing)
    keys_ms = [key for key in runs[0] if key.endswith("_ms")] + ["host_workers"]
    mean = {key: float(np.mean([r[key] for r in runs])) for key in keys_ms + ["frame_bytes", "coeff_blocks"]}
    out = {"config": args.config, "frames": n, "macroblocks": nmb, "reps": args.reps, "runs": runs, "mean": mean,
           "bytes_per_macroblock_written": mean["frame_bytes"] / nmb, "bytes_per_macroblock_rebase_download": 804,
           "macroblocks_per_s_serialize_call": nmb / mean["serialize_call_ms"] * 1e3, "macroblocks_per_s_token_kernel": nmb / mean["serialize_kernel_ms"] * 1e3}
    print("rebase of %d frames (%d macroblocks): call %.1f ms = up + kernels %.1f, download %.1f, host records %.1f, append %.1f"
          % (n, nmb, mean["rebase_call_ms"], mean["rebase_kernels_ms"], mean["rebase_download_ms"], mean["rebase_records_ms"], mean["rebase_append_ms"]), flush=True)
    print("serialise of the same frames: call %.1f ms = up + k_serialize_tokens %.1f, sizes + partitions down %.1f, host first partitions %.1f (beside the kernel), assembly + copy %.1f; "
          "%.1f bytes per macroblock written (the rebase downloads 804); %.2f M macroblocks/s through the token kernel"
          % (mean["serialize_call_ms"], mean["serialize_kernel_ms"], mean["serialize_download_ms"], mean["serialize_first_partition_ms"], mean["serialize_assemble_ms"],
             out["bytes_per_macroblock_written"], out["macroblocks_per_s_token_kernel"] / 1e6), flush=True)
    print("the same %d frames by the host: %.1f ms on %d worker threads (one frame alone on one core: %.1f ms); the GPU's token kernel: %.1f ms"
          % (n, mean["host_serialize_ms"], int(mean["host_workers"]), mean["host_one_frame_one_core_ms"], mean["serialize_kernel_ms"]), flush=True)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
