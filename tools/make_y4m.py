#!/usr/bin/env python3
"""Deterministic synthetic source video written as YUV4MPEG2 C420jpeg.

luma = 128 + 50 sin(x/a) + 40 cos(y/b) + 20 sin((x+y)/c) + texture, sampled from a
(W+64)x(H+64) canvas translated by (3n mod 64, 2n mod 64) per frame (real sub-pel motion
once the encoder searches it), plus per-pixel uniform noise.  Test/bench tooling only.
"""
import argparse
import numpy as np


def synth_frames(width, height, frames, seed, entropy="low"):
    rng = np.random.default_rng(seed)
    if entropy == "low":
        a, b, c, tex, noise = 37.0, 23.0, 11.0, 12, 3
    else:
        a, b, c, tex, noise = 7.0, 5.0, 11.0, 40, 10
    cw, ch = width + 64, height + 64
    x = np.arange(cw)[None, :]
    y = np.arange(ch)[:, None]
    canvas = 128 + 50 * np.sin(x / a) + 40 * np.cos(y / b) + 20 * np.sin((x + y) / c)
    canvas = canvas + rng.integers(-tex, tex + 1, size=(ch, cw))
    cu = 128 + 30 * np.sin(x[:, ::2] / 29.0) + 20 * np.cos(y[::2, :] / 31.0)
    cv = 128 + 30 * np.cos(x[:, ::2] / 19.0) + 20 * np.sin(y[::2, :] / 41.0)
    for n in range(frames):
        ox, oy = (3 * n) % 64, (2 * n) % 64
        Y = canvas[oy:oy + height, ox:ox + width] + rng.integers(-noise, noise + 1, size=(height, width))
        cwid, chei = (width + 1) // 2, (height + 1) // 2
        U = cu[oy // 2:oy // 2 + chei, ox // 2:ox // 2 + cwid]
        V = cv[oy // 2:oy // 2 + chei, ox // 2:ox // 2 + cwid]
        yield (np.clip(Y, 0, 255).astype(np.uint8), np.clip(U, 0, 255).astype(np.uint8),
               np.clip(V, 0, 255).astype(np.uint8))


CRAFTED_FAMILIES = ("noise", "checker", "sparse", "dot")


def crafted(width, height, family, amp, cell, base, gx, gy, salt):
    """A crafted still picture -> (Y, U, V) uint8: a luma ramp (gx, gy: quarter levels per pixel) under one of four textures, flat
    chroma with one level of ripple.  Integer arithmetic only and no generator state, so that every caller gets the same bytes.  The
    pictures of synth_frames never bring the reference's second pass to empty a Y2 block or to choose B_PRED after a 16x16 mode; some
    of these do (tests/golden/make_two_pass_crafted_golden.py)."""
    assert family in CRAFTED_FAMILIES and amp >= 1 and cell >= 1
    x = np.arange(width, dtype=np.int64)[None, :]
    y = np.arange(height, dtype=np.int64)[:, None]
    hsh = ((x // cell) * 2654435761 ^ (y // cell) * 40503 ^ salt * 97) & 0xffffffff
    hsh ^= hsh >> 13
    hsh = hsh * 0x5bd1e995 & 0xffffffff
    hsh ^= hsh >> 15
    v = base + gx * x // 4 + gy * y // 4
    if family == "noise":
        v = v + hsh % amp
    elif family == "checker":
        v = v + ((x // cell + y // cell) & 1) * amp
    elif family == "sparse":
        v = v + np.where(hsh % 8 == 0, amp, 0)
    else:
        v = v + np.where(((x % 16) // 4 == 1) & ((y % 16) // 4 == 2), amp, 0)
    Y = np.clip(v, 0, 255).astype(np.uint8)
    U = np.full(((height + 1) // 2, (width + 1) // 2), 128, np.uint8)
    V = U.copy()
    U[::2, ::3] += 1
    return Y, U, V


def crafted_frames(width, height, frames, family, amp, cell, base, gx, gy, salt):
    """The same crafted picture for every frame index."""
    for _ in range(frames):
        yield crafted(width, height, family, amp, cell, base, gx, gy, salt)


def write_y4m_frames(path, width, height, pictures, fps=30):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F%d:1 Ip A1:1 C420jpeg\n" % (width, height, fps))
        for Y, U, V in pictures:
            f.write(b"FRAME\n")
            f.write(Y.tobytes()); f.write(U.tobytes()); f.write(V.tobytes())


def write_y4m(path, width, height, frames, seed, entropy="low", fps=30):
    write_y4m_frames(path, width, height, synth_frames(width, height, frames, seed, entropy), fps)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out"); ap.add_argument("--width", type=int, default=176)
    ap.add_argument("--height", type=int, default=144); ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--seed", type=int, default=7); ap.add_argument("--entropy", default="low")
    ap.add_argument("--fps", type=int, default=30)
    a = ap.parse_args()
    write_y4m(a.out, a.width, a.height, a.frames, a.seed, a.entropy, a.fps)
