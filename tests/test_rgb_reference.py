"""The RGB conversion's definition (tests/rgb_reference.py) against the reference display's shader (display.cc: GL bilinear
sampling of the chroma textures, SMPTE 170M matrix in floating point), and the library's export of the entry point."""
import numpy as np
import pytest

import rgb_reference as rr

# the shader's real-valued matrix (display.cc, shader_source_ycbcr), on 0..1 values
K_Y, OFF_Y, OFF_C = 1.16438356164384, 0.06274509803921568627, 0.50196078431372549019
K_RV, K_GU, K_GV, K_BU = 1.59567019581339, 0.391260370716072, 0.813004933873461, 2.01741475897078


def gl_bilinear8(c, width, height):
    """GL_LINEAR sampling with clamp-to-edge of a (h+1)/2 x (w+1)/2 texture at the chroma coordinates display.cc gives a fragment
    centre (x + 0.5, y + 0.5): ((x + 0.5) / 2 + 0.25, (y + 0.5) / 2), in float64, times 8."""
    cw, ch = (width + 1) // 2, (height + 1) // 2
    tex = np.asarray(c, np.float64)[:ch, :cw]
    s = (np.arange(width) + 0.5) / 2 + 0.25 - 0.5             # texel space: texel centres at integers
    t = (np.arange(height) + 0.5) / 2 - 0.5
    i0, j0 = np.floor(t).astype(int), np.floor(s).astype(int)
    a, b = t - i0, s - j0
    ia, ib = np.clip(i0, 0, ch - 1), np.clip(i0 + 1, 0, ch - 1)
    ja, jb = np.clip(j0, 0, cw - 1), np.clip(j0 + 1, 0, cw - 1)
    top = tex[ia][:, ja] * (1 - b) + tex[ia][:, jb] * b
    bot = tex[ib][:, ja] * (1 - b) + tex[ib][:, jb] * b
    return 8 * (top * (1 - a)[:, None] + bot * a[:, None])


@pytest.mark.parametrize("w,h", [(33, 17), (175, 143), (64, 64)])
def test_chroma_upsampling_equals_gl_bilinear_sampling(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    pw, ph = 16 * ((w + 15) // 16), 16 * ((h + 15) // 16)
    c = rng.integers(0, 256, (ph // 2, pw // 2), dtype=np.uint8)
    got = rr.upsample_chroma8(c, w, h)
    want = gl_bilinear8(c, w, h)
    assert got.shape == (h, w)
    assert np.array_equal(got, want)                            # dyadic weights: exact in float64


def _real(Y, cb8, cr8):
    y = K_Y * (Y / 255.0 - OFF_Y)
    cb, cr = cb8 / 2040.0 - OFF_C, cr8 / 2040.0 - OFF_C
    clip = lambda q: np.clip(np.floor(np.clip(q, 0, 1) * 255 + 0.5), 0, 255)
    return clip(y + K_RV * cr), clip(y - K_GU * cb - K_GV * cr), clip(y + K_BU * cb)


def test_integer_matrix_within_one_of_the_shader_for_red_and_blue_exhaustively():
    Y, C8 = np.meshgrid(np.arange(256), np.arange(2041), indexing="ij")
    Y, C8 = Y.ravel(), C8.ravel()
    mid = np.full_like(C8, 1024)
    r, _, _ = rr.matrix(Y, mid, C8)
    rr_, _, _ = _real(Y, mid, C8)
    d = np.abs(r.astype(int) - rr_.astype(int))
    assert d.max() <= 1 and 0 < np.count_nonzero(d) < 100
    _, _, b = rr.matrix(Y, C8, mid)
    _, _, br = _real(Y, C8, mid)
    d = np.abs(b.astype(int) - br.astype(int))
    assert d.max() <= 1 and 0 < np.count_nonzero(d) < 100


def test_integer_matrix_within_one_of_the_shader_for_green_on_random_triples():
    rng = np.random.default_rng(170)
    for _ in range(10):
        n = 1_000_000
        Y, cb, cr = rng.integers(0, 256, n), rng.integers(0, 2041, n), rng.integers(0, 2041, n)
        _, g, _ = rr.matrix(Y, cb, cr)
        _, gr, _ = _real(Y, cb, cr)
        d = np.abs(g.astype(int) - gr.astype(int))
        assert d.max() <= 1
        assert np.count_nonzero(d) < n * 0.001


@pytest.mark.parametrize("fmt", ["chw_f16", "chw_bf16", "chw_f32"])
@pytest.mark.parametrize("mean,std", [(None, None), ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), ((0.5, -3.0, 1e-3), (1e-6, 7.0, -0.5))])
def test_float_tables_follow_double_float32_dtype_rounding(fmt, mean, std):
    t = rr.table(fmt, mean, std)
    m = np.zeros(3) if mean is None else np.array(mean)
    s = np.ones(3) if std is None else np.array(std)
    for c in range(3):
        for i in (0, 1, 17, 128, 254, 255):
            f32 = np.float32((i / 255.0 - m[c]) / s[c])
            if fmt == "chw_f32":
                assert t[c][i] == f32.view(np.uint32)
            elif fmt == "chw_f16":
                with np.errstate(over="ignore"):
                    assert t[c][i] == np.float16(f32).view(np.uint16)
            else:
                import torch
                assert t[c][i] == torch.tensor([float(f32)], dtype=torch.float32).to(torch.bfloat16).view(torch.int16).item() & 0xFFFF


def test_library_exports_render_rgb():
    import ctypes
    from alfalfa_amd import build as b
    b.build()
    lib = ctypes.CDLL(b.LIB)
    assert hasattr(lib, "aa_render_rgb_async")
    from alfalfa_amd import capi
    assert any(name == "aa_render_rgb_async" for name, _, _ in capi.SYMBOLS)


def test_torch_imported_after_the_library_shares_its_hip_runtime():
    """Context.to_rgb hands torch tensors to the library: both must run on ONE HIP runtime in the process (a second one, started by
    torch's own copies of the runtime libraries, finds no GPU)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from alfalfa_amd import capi; capi.lib()\n"
            "import torch\n"
            "maps = open('/proc/self/maps').read().splitlines()\n"
            "print(sorted({l.split()[-1].rsplit('/', 1)[0] for l in maps if 'libamdhip64' in l or 'libhsa-runtime64' in l}))" % root)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    assert len(eval(out)) == 1, out
