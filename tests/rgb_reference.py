"""numpy restatement of the RGB conversion (aa_render_rgb_async, INTEGRATION.md "Frames as RGB"): the contract the GPU kernel is
tested against, bit for bit.  Input: the padded planes of Decoder.raster(); output: the display rectangle in one of the formats."""
import numpy as np

CY, CRV, CGU, CGV, CBU = 76309, 104574, 25642, 53281, 132213

FORMATS = ("rgb24", "rgba", "chw_u8", "chw_f16", "chw_bf16", "chw_f32")


def upsample_chroma8(c, width, height):
    """Chroma plane (padded) -> height x width at 8x scale: co-sited horizontally, centred vertically, clamp-to-edge inside the
    display chroma rectangle ((width+1)/2 x (height+1)/2)."""
    cw, ch = (width + 1) // 2, (height + 1) // 2
    c = np.asarray(c)[:ch, :cw].astype(np.int32)
    y = np.arange(height)
    k = y >> 1
    kn = np.where(y & 1, np.minimum(k + 1, ch - 1), np.maximum(k - 1, 0))
    v = 3 * c[k] + c[kn]                                       # 4x scale
    x = np.arange(width)
    j, jn = x >> 1, np.minimum((x >> 1) + 1, cw - 1)
    return np.where(x & 1, v[:, j] + v[:, jn], 2 * v[:, j])    # 8x scale, 0..2040


def matrix(Y, cb8, cr8):
    """Integer SMPTE 170M limited-range matrix: -> R, G, B (uint8 arrays)."""
    yt = 8 * CY * (np.asarray(Y, np.int32) - 16)
    ut, vt = np.asarray(cb8, np.int32) - 1024, np.asarray(cr8, np.int32) - 1024
    r = (yt + CRV * vt + (1 << 18)) >> 19
    g = (yt - CGU * ut - CGV * vt + (1 << 18)) >> 19
    b = (yt + CBU * ut + (1 << 18)) >> 19
    return tuple(np.clip(q, 0, 255).astype(np.uint8) for q in (r, g, b))


def rgb_u8(planes, width, height):
    """-> (height, width, 3) uint8."""
    y, u, v = planes
    r, g, b = matrix(np.asarray(y)[:height, :width], upsample_chroma8(u, width, height), upsample_chroma8(v, width, height))
    return np.stack([r, g, b], axis=-1)


def bf16_bits(f32):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even."""
    b = np.asarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def table(fmt, mean=None, std=None):
    """3 x 256 output values of a float format as bit patterns (uint16 for f16 / bf16, uint32 for f32)."""
    mean = np.zeros(3) if mean is None else np.asarray(mean, np.float64)
    std = np.ones(3) if std is None else np.asarray(std, np.float64)
    i = np.arange(256, dtype=np.float64) / 255.0
    t32 = ((i[None, :] - mean[:, None]) / std[:, None]).astype(np.float32)
    if fmt == "chw_f32":
        return t32.view(np.uint32)
    if fmt == "chw_f16":
        with np.errstate(over="ignore"):
            return t32.astype(np.float16).view(np.uint16)
    if fmt == "chw_bf16":
        return bf16_bits(t32)
    raise ValueError(fmt)


def expected(planes, width, height, fmt, mean=None, std=None):
    """The output of one frame: uint8 (H, W, 3|4) / (3, H, W); float formats as bit patterns (uint16 / uint32) of (3, H, W)."""
    rgb = rgb_u8(planes, width, height)
    if fmt == "rgb24":
        return rgb
    if fmt == "rgba":
        return np.concatenate([rgb, np.full((height, width, 1), 255, np.uint8)], axis=-1)
    chw = np.ascontiguousarray(rgb.transpose(2, 0, 1))
    if fmt == "chw_u8":
        return chw
    t = table(fmt, mean, std)
    return np.stack([t[c][chw[c]] for c in range(3)])


def as_bits(a):
    """numpy view of a rendered tensor's host copy in the form expected() returns (bit patterns for float formats)."""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype in (np.float16, np.int16):
        return a.view(np.uint16)
    return a
