"""The forward path of the rebase (Encoder::update_residues, reencode.cc:131-303) restated in numpy with plain loops, and the loaders of
the fixtures under tests/golden/rebase (written by the reference: tests/golden/make_rebase_golden.py).  Test support, no product code:

  fdct / wht / quantize            what DCTCoefficients::subtract_dct, ::wht (dct.cc:45-163, the C++ branch) and ::quantize
                                   (quantization.cc:148-157) compute -- tests/test_rebase_model.py pins them to the reference's own output,
                                   tests/cpp/forward_math_check.cc pins vp8_math.hh to them
  luma_of_whole_pel_macroblock     coefficients of a non-split inter macroblock with a whole-pel vector
  load_case / parse_frames / dense fixture access through the product's host parser"""
import json
import os

import numpy as np

import alfalfa_amd as aa
import vp8_oracle as vo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rebase")
HASHES = json.load(open(os.path.join(GOLDEN, "rebase_golden.json")))
ENC_CASES = ["enc_rt_64x48", "enc_best_72x40", "enc_skip_80x48"]
DIR_CASES = ["dir_split_80x48", "dir_fraction_80x48", "dir_edge_80x48", "dir_wave_80x48", "dir_split_16x16"]
CASES = ENC_CASES + DIR_CASES
B_PRED, SPLITMV = 4, 9


def i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def fdct(res):
    """res: 4x4 (rows, columns) of target - prediction -> the 16 coefficients in raster order."""
    im = [0] * 16
    for r in range(4):
        a1, b1 = (int(res[r][0]) + int(res[r][3])) * 8, (int(res[r][1]) + int(res[r][2])) * 8
        c1, d1 = (int(res[r][1]) - int(res[r][2])) * 8, (int(res[r][0]) - int(res[r][3])) * 8
        im[4 * r + 0], im[4 * r + 2] = i16(a1 + b1), i16(a1 - b1)
        im[4 * r + 1] = i16((c1 * 2217 + d1 * 5352 + 14500) >> 12)
        im[4 * r + 3] = i16((d1 * 2217 - c1 * 5352 + 7500) >> 12)
    out = [0] * 16
    for i in range(4):
        a1, b1, c1, d1 = im[i] + im[i + 12], im[i + 4] + im[i + 8], im[i + 4] - im[i + 8], im[i] - im[i + 12]
        out[i], out[i + 8] = i16((a1 + b1 + 7) >> 4), i16((a1 - b1 + 7) >> 4)
        out[i + 4] = i16(((c1 * 2217 + d1 * 5352 + 12000) >> 16) + (1 if d1 != 0 else 0))
        out[i + 12] = i16((d1 * 2217 - c1 * 5352 + 51000) >> 16)
    return out


def wht(dcs):
    """dcs: the 16 luma DCs, raster order -> the 16 Y2 coefficients."""
    im = [0] * 16
    for r in range(4):
        i0, i1, i2, i3 = (int(dcs[4 * r + k]) for k in range(4))
        a1, d1, c1, b1 = (i0 + i2) * 4, (i1 + i3) * 4, (i1 - i3) * 4, (i0 - i2) * 4
        im[4 * r + 0], im[4 * r + 1], im[4 * r + 2], im[4 * r + 3] = i16(a1 + d1 + (1 if a1 != 0 else 0)), i16(b1 + c1), i16(b1 - c1), i16(a1 - d1)
    out = [0] * 16
    for i in range(4):
        a1, d1, c1, b1 = im[i] + im[i + 8], im[i + 4] + im[i + 12], im[i + 4] - im[i + 12], im[i] - im[i + 8]
        for k, x in ((0, a1 + d1), (4, b1 + c1), (8, b1 - c1), (12, a1 - d1)):
            out[i + k] = i16((x + (1 if x < 0 else 0) + 3) >> 3)
    return out


def quantize(coeffs, fdc, fac):
    """Integer division truncating toward zero: index 0 by the DC factor, 1..15 by the AC factor."""
    def div(a, b):
        return -((-a) // b) if a < 0 else a // b
    return [i16(div(int(c), fdc if i == 0 else fac)) for i, c in enumerate(coeffs)]


def luma_of_whole_pel_macroblock(target_y, ref_y, col, row, mv, quant):
    """Non-split inter macroblock (col, row) with the whole-pel vector mv = (x, y) in quarter pels: prediction = the reference block at
    the vector with coordinates clamped to the plane -> (luma [16][16], DCs zeroed before the division; Y2 [16])."""
    ph, pw = ref_y.shape
    ys = np.clip(np.arange(16) + row * 16 + (mv[1] >> 3), 0, ph - 1)
    xs = np.clip(np.arange(16) + col * 16 + (mv[0] >> 3), 0, pw - 1)
    res = target_y[row * 16:row * 16 + 16, col * 16:col * 16 + 16].astype(np.int32) - ref_y[np.ix_(ys, xs)].astype(np.int32)
    luma, dcs = [], []
    for b in range(16):
        c = fdct(res[(b >> 2) * 4:(b >> 2) * 4 + 4, (b & 3) * 4:(b & 3) * 4 + 4])
        dcs.append(c[0])
        c[0] = 0
        luma.append(quantize(c, quant[0], quant[1]))
    return luma, quantize(wht(dcs), quant[2], quant[3])


# ---- fixtures ----
def load_case(name):
    """-> dict: w, h, pw, ph, state (bytes), pred / rebased (frames), targets ([(y, u, v)] padded and edge-extended), sha256 ([hex])."""
    d = os.path.join(GOLDEN, name)
    g = HASHES[name]
    w, h = g["width"], g["height"]
    pw, ph = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    raw = np.fromfile(os.path.join(d, "target.yuv"), np.uint8)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    fs = w * h + 2 * cw * ch
    assert len(raw) == fs * g["frames"]
    targets = []
    for k in range(g["frames"]):
        f = raw[k * fs:(k + 1) * fs]
        y, u, v = f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:].reshape(ch, cw)
        targets.append((np.pad(y, ((0, ph - h), (0, pw - w)), mode="edge"), np.pad(u, ((0, ph // 2 - ch), (0, pw // 2 - cw)), mode="edge"),
                        np.pad(v, ((0, ph // 2 - ch), (0, pw // 2 - cw)), mode="edge")))
    case = {"name": name, "w": w, "h": h, "pw": pw, "ph": ph, "state": open(os.path.join(d, "c0.state"), "rb").read(),
            "pred": vo.read_ivf(os.path.join(d, "pred.ivf"))[2], "rebased": vo.read_ivf(os.path.join(d, "rebased.ivf"))[2],
            "targets": targets, "sha256": g["raster_sha256"]}
    if os.path.exists(os.path.join(d, "c0.ivf")):
        case["c0"] = vo.read_ivf(os.path.join(d, "c0.ivf"))[2]
    assert len(case["pred"]) == len(case["rebased"]) + 1 == g["frames"] + 1
    return case


def state_raster(case):
    """The LAST reference of c0.state (Decoder::serialize, decoder.cc:54-69: the padded planes are the file's tail) -> (y, u, v)."""
    pw, ph = case["pw"], case["ph"]
    tail = np.frombuffer(case["state"][-(pw * ph * 3 // 2):], np.uint8)
    return tail[:pw * ph].reshape(ph, pw), tail[pw * ph:pw * ph * 5 // 4].reshape(ph // 2, pw // 2), tail[pw * ph * 5 // 4:].reshape(ph // 2, pw // 2)


def decoder_state(case):
    """The DecoderState part of c0.state: [DECODER][u32] DecoderState [REFERENCES][u32][u16 w][u16 h][REF_LAST][u32] planes."""
    return case["state"][5:len(case["state"]) - (14 + case["pw"] * case["ph"] * 3 // 2)]


def parse_frames(case, which):
    """The product's host parser over pred.ivf (from its key frame) or rebased.ivf (continuing from c0.state) -> [(header, mb, blocks)]."""
    p = aa.Parser(case["w"], case["h"])
    if which == "rebased":
        p.deserialize_state(decoder_state(case))
    return [p.parse(fr) for fr in case[which]]


def dense(mb, blocks):
    """A frame's records -> [mbh, mbw, 25, 16] (slot 24 = Y2), zero where nothing is stored."""
    mbh, mbw = mb.shape
    out = np.zeros((mbh, mbw, 25, 16), np.int16)
    for r in range(mbh):
        for c in range(mbw):
            m, k = int(mb[r, c]["nz_mask"]), int(mb[r, c]["coeff_index"])
            for b in [24] + list(range(24)):
                if (m >> b) & 1:
                    out[r, c, b] = blocks[k]
                    k += 1
    return out


def vectors(rec):
    return np.frombuffer(rec["u"].tobytes(), "<i2").reshape(16, 2)


def describe(rec):
    """A macroblock's class, for failure messages."""
    if rec["ref_frame"] == 0:
        return "intra B_PRED" if rec["y_mode"] == B_PRED else "intra 16x16 mode %d" % rec["y_mode"]
    mv = vectors(rec)
    if rec["y_mode"] == SPLITMV:
        return "SPLITMV partition %d ref %d" % (rec["split_partition"], rec["ref_frame"])
    fx, fy = int(mv[0][0]) & 7, int(mv[0][1]) & 7
    return "inter ref %d mv (%d, %d) %s" % (rec["ref_frame"], mv[0][0], mv[0][1], "whole-pel" if not (fx or fy) else "sub-pel " + ("x" if fx else "") + ("y" if fy else ""))
