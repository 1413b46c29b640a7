"""The JPEG round trip of the SISR degradation: what ``cv2.imencode('.jpg', im, [IMWRITE_JPEG_QUALITY, qf])`` followed by ``cv2.imdecode``
does to an 8-bit RGB image (utils/util_image.py:236-257, the last step of utils/util_sisr.py:146-177 and of datasets/SISRDatasets.py:107-112),
restated as integer arithmetic.  The entropy coding is lossless and drops out; what is left is libjpeg's baseline path with the library's
defaults (4:2:0 sampling, "slow integer" DCT, "fancy" upsampling, ``force_baseline``), every step of which decides bytes:

 1. RGB -> YCbCr in 16-bit fixed point, ``F(x) = round(x * 65536)``:
      ``Y  = (F(.299) R + F(.587) G + F(.114) B + 32768) >> 16``
      ``Cb = (-F(.16874) R - F(.33126) G + 32768 B + (128 << 16) + 32767) >> 16``
      ``Cr = (32768 R - F(.41869) G - F(.08131) B + (128 << 16) + 32767) >> 16``
 2. Padding by edge replication.  Y: to multiples of 8.  Chroma, with ``hc = ceil(H/2)``, ``wc = ceil(W/2)``: the full-resolution plane is
    replicated to ``2 hc`` rows and ``2 * 8 ceil(wc/8)`` columns and downsampled; the last DOWNSAMPLED row is then replicated down to a
    multiple of 8.  (Rows replicated before and after the downsampling differ when H is even, and they share a DCT block with real rows.)
 3. 2 x 2 chroma downsample ``(a + b + c + d + bias) >> 2``, the bias alternating 1, 2, 1, 2, ... along a row from 1 in column 0.
 4. Forward DCT of ``sample - 128`` in the Loeffler-Ligtenberg-Moshovitz form with 13 constant bits and 2 pass-1 bits, rows then columns;
    every descale is ``(x + (1 << (n - 1))) >> n`` with an arithmetic shift.  The result is the DCT scaled by 8.
 5. Quantise with the divisor ``8 q``: ``sign(c) * ((|c| + (8 q >> 1)) // (8 q))``; dequantise by ``* q``.  The tables are those of the
    JPEG specification's Annex K scaled by the quality (:func:`quant_tables`).
 6. Inverse DCT of the same family, columns then rows, descales by 11 and 18 bits, ``+ 128``, clip to 0..255.  (The library's DC-only
    shortcut gives the same values as the general path.)
 7. Chroma "fancy" 2x upsample of the ``hc x wc`` plane cropped from the padded blocks.  Vertically ``v = 3 near + far`` (the row above
    row 0 is row 0, the row below the last row is the last row); horizontally the even output is ``(3 v[j] + v[j-1] + 8) >> 4`` and the
    odd one ``(3 v[j] + v[j+1] + 7) >> 4``, the first and last columns standing in for their own missing neighbour.  Crop to H x W.
    The library picks this filter only for planes more than two samples wide: with ``wc <= 2`` (W <= 4) each chroma sample is
    repeated 2 x 2 instead.
 8. YCbCr -> RGB in 16-bit fixed point with cb, cr centred at 128, clipped to 0..255:
      ``R = Y + ((F(1.402) cr + 32768) >> 16)``,  ``B = Y + ((F(1.772) cb + 32768) >> 16)``,
      ``G = Y + ((-F(.34414) cb - F(.71414) cr + 32768) >> 16)``

:func:`roundtrip_np` is that definition on the host (numpy, int64); tests/golden/jpeg.npz pins it to Pillow's libjpeg-turbo byte for byte.
OpenCV was not available to compare with: that its output equals Pillow's rests on both bundling libjpeg-turbo and using its defaults.

:func:`jpeg_compress` is the same on the device (csrc/jpeg.hip) for a batch of CUDA images with one quality per sample; quality 0 leaves a
sample untouched, which is what the 'Gaussian' samples of a mixed training batch need.  Every intermediate fits 32 bits, as the library
was designed.  Results are bitwise reproducible and do not depend on the batch an image sits in; nothing synchronises, the two launches go
on the current stream.  The first call per device uploads the table of all 100 qualities' divisors: warm a device up before capturing a
graph; after that a call whose ``qf`` is a tensor copies nothing from the host.
"""
from __future__ import annotations

import functools
from typing import Tuple

import numpy as np

# JPEG specification, Annex K, tables K.1 and K.2, in natural (row-major) order
_BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
_BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64).reshape(8, 8)


def quant_tables(qf: int) -> Tuple[np.ndarray, np.ndarray]:
    """(luma, chroma) int32 [8,8] divisors of quality ``qf`` (clipped to 1..100), natural order."""
    q = min(max(int(qf), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int32) for base in (_BASE_LUMA, _BASE_CHROMA))


def all_quant_tables() -> np.ndarray:
    """int32 [101, 2, 64]: entry q holds quality q's (luma, chroma) divisors; entry 0 is unused (zeros)."""
    out = np.zeros((101, 2, 64), dtype=np.int32)
    for q in range(1, 101):
        luma, chroma = quant_tables(q)
        out[q, 0], out[q, 1] = luma.reshape(-1), chroma.reshape(-1)
    return out


# ---- the DCT pair (13 constant bits, 2 pass-1 bits) -----------------------------------------------------------------------------------
_CONST_BITS, _PASS1_BITS = 13, 2
_F0_298, _F0_390, _F0_541, _F0_765, _F0_899, _F1_175 = 2446, 3196, 4433, 6270, 7373, 9633
_F1_501, _F1_847, _F1_961, _F2_053, _F2_562, _F3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n: int):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d: np.ndarray, first: bool) -> np.ndarray:
    """One pass along the last axis of [..., 8] int64."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = _CONST_BITS - _PASS1_BITS if first else _CONST_BITS + _PASS1_BITS
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << _PASS1_BITS, (t10 - t11) << _PASS1_BITS
    else:
        out[0], out[4] = _descale(t10 + t11, _PASS1_BITS), _descale(t10 - t11, _PASS1_BITS)
    z1 = (t12 + t13) * _F0_541
    out[2] = _descale(z1 + t13 * _F0_765, n)
    out[6] = _descale(z1 - t12 * _F1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _F1_175
    t4, t5, t6, t7 = t4 * _F0_298, t5 * _F2_053, t6 * _F3_072, t7 * _F1_501
    z1, z2, z3, z4 = -z1 * _F0_899, -z2 * _F2_562, -z3 * _F1_961 + z5, -z4 * _F0_390 + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def _idct_pass(c: np.ndarray, n: int) -> np.ndarray:
    """One pass along the last axis of [..., 8] int64, descaled by ``n`` bits."""
    c0, c1, c2, c3, c4, c5, c6, c7 = (c[..., i] for i in range(8))
    z1 = (c2 + c6) * _F0_541
    t2, t3 = z1 - c6 * _F1_847, z1 + c2 * _F0_765
    t0, t1 = (c0 + c4) << _CONST_BITS, (c0 - c4) << _CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c7, c5, c3, c1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * _F1_175
    t0, t1, t2, t3 = t0 * _F0_298, t1 * _F2_053, t2 * _F3_072, t3 * _F1_501
    z1, z2, z3, z4 = -z1 * _F0_899, -z2 * _F2_562, -z3 * _F1_961 + z5, -z4 * _F0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([_descale(t10 + t3, n), _descale(t11 + t2, n), _descale(t12 + t1, n), _descale(t13 + t0, n),
                     _descale(t13 - t0, n), _descale(t12 - t1, n), _descale(t11 - t2, n), _descale(t10 - t3, n)], axis=-1)


def _plane_roundtrip(plane: np.ndarray, table: np.ndarray) -> np.ndarray:
    """Steps 4-6 on a plane whose sides are multiples of 8: int64 [h,w] samples 0..255 -> the same."""
    h, w = plane.shape
    blk = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)            # [by, bx, row, col]
    coef = _fdct_pass(blk, True)                                                       # rows
    coef = _fdct_pass(coef.swapaxes(-1, -2), False).swapaxes(-1, -2)                   # columns
    div = table.astype(np.int64) * 8
    quant = np.sign(coef) * ((np.abs(coef) + (div >> 1)) // div)
    coef = quant * table.astype(np.int64)
    ws = _idct_pass(coef.swapaxes(-1, -2), _CONST_BITS - _PASS1_BITS).swapaxes(-1, -2)  # columns
    out = _idct_pass(ws, _CONST_BITS + _PASS1_BITS + 3)                                 # rows
    out = np.clip(out + 128, 0, 255)
    return out.transpose(0, 2, 1, 3).reshape(h, w)


def _pad_edge(a: np.ndarray, h: int, w: int) -> np.ndarray:
    return np.pad(a, ((0, h - a.shape[0]), (0, w - a.shape[1])), mode="edge")


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


def roundtrip_np(im: np.ndarray, qf: int) -> np.ndarray:
    """The definition: uint8 [h,w,3] RGB -> uint8 [h,w,3], the decoded baseline JPEG of quality ``qf`` (clipped to 1..100)."""
    im = np.asarray(im)
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
        raise TypeError(f"roundtrip_np expects a uint8 [h,w,3] image, got {im.dtype} {im.shape}")
    h, w = im.shape[:2]
    if h == 0 or w == 0:
        raise ValueError(f"roundtrip_np: empty image {im.shape}")
    luma, chroma = quant_tables(qf)
    r, g, b = (im[:, :, i].astype(np.int64) for i in range(3))
    # 1
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    # 2-6
    hc, wc = -(-h // 2), -(-w // 2)
    y = _plane_roundtrip(_pad_edge(y, -(-h // 8) * 8, -(-w // 8) * 8), luma)[:h, :w]
    bias = np.tile(np.array([1, 2], dtype=np.int64), 4 * -(-wc // 8))
    small = []
    for c in (cb, cr):
        full = _pad_edge(c, 2 * hc, 16 * -(-wc // 8))
        down = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] + bias) >> 2
        small.append(_plane_roundtrip(_pad_edge(down, -(-hc // 8) * 8, down.shape[1]), chroma)[:hc, :wc])
    # 7
    up = []
    for c in small:
        if wc <= 2:
            up.append(np.repeat(np.repeat(c, 2, 0), 2, 1)[:h, :w])
            continue
        above, below = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
        v = np.empty((2 * hc, wc), dtype=np.int64)
        v[0::2], v[1::2] = 3 * c + above, 3 * c + below
        left, right = np.concatenate([v[:, :1], v[:, :-1]], 1), np.concatenate([v[:, 1:], v[:, -1:]], 1)
        out = np.empty((2 * hc, 2 * wc), dtype=np.int64)
        out[:, 0::2], out[:, 1::2] = (3 * v + left + 8) >> 4, (3 * v + right + 7) >> 4
        up.append(out[:h, :w])
    # 8
    cb, cr = up[0] - 128, up[1] - 128
    rgb = np.stack([y + ((_fix(1.402) * cr + 32768) >> 16),
                    y + ((-_fix(.34414) * cb - _fix(.71414) * cr + 32768) >> 16),
                    y + ((_fix(1.772) * cb + 32768) >> 16)], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


# ---- the device path (csrc/jpeg.hip) ------------------------------------------------------------------------------------------------------
# torch and the native library are imported on first use: the host definition above (eval.jpeg_compress) needs numpy only
MAX_BATCH, MAX_SIDE = 65535, 32768


@functools.lru_cache(maxsize=16)
def _device_tables(device: str):
    """The [101,2,64] int32 divisor table on ``device``, uploaded once."""
    import torch
    from . import _native
    with _native.capture_lock:
        return torch.from_numpy(all_quant_tables()).to(torch.device(device))


def warm(device) -> None:
    """Upload the divisor table of ``device`` ahead of time (before a graph capture, or outside a timed region)."""
    import torch
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    _device_tables(str(dev))


def _check_args(x, qf):
    """All checks before any device work.  Returns ``qf`` as an int, a list of ints or the int32 CUDA tensor it is."""
    import torch
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a tensor, got {type(x).__name__}")
    if x.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"x must be uint8 or float32, got {x.dtype}")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"x must be [N,3,H,W], got {tuple(x.shape)}")
    n, _, h, w = x.shape
    if not 1 <= n <= MAX_BATCH:
        raise ValueError(f"batch {n} outside 1..{MAX_BATCH}")
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"image {h}x{w} outside 1..{MAX_SIDE}")
    if isinstance(qf, torch.Tensor):
        if qf.dtype != torch.int32:
            raise TypeError(f"a tensor qf must be int32, got {qf.dtype}")
        if tuple(qf.shape) != (n,):
            raise ValueError(f"a tensor qf must be [{n}], one quality per sample, got {tuple(qf.shape)}")
    elif isinstance(qf, (bool, float, str, bytes)) or qf is None:
        raise TypeError(f"qf must be an int, a sequence of ints or an int32 tensor, got {type(qf).__name__}")
    elif isinstance(qf, (int, np.integer)):
        qf = int(qf)
        if not 0 <= qf <= 100:
            raise ValueError(f"qf {qf}: 0 (no compression) or a quality 1..100")
    else:
        try:
            vals = list(qf)
        except TypeError:
            raise TypeError(f"qf must be an int, a sequence of ints or an int32 tensor, got {type(qf).__name__}") from None
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in vals):
            raise TypeError("qf must hold ints")
        if len(vals) != n:
            raise ValueError(f"qf has {len(vals)} entries for a batch of {n}: one quality per sample")
        qf = [int(v) for v in vals]
        if any(not 0 <= v <= 100 for v in qf):
            raise ValueError(f"qf {qf}: every entry 0 (no compression) or a quality 1..100")
    if not x.is_cuda:
        raise RuntimeError(f"x is on {x.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    if isinstance(qf, torch.Tensor) and qf.device != x.device:
        raise RuntimeError(f"x is on {x.device}, qf on {qf.device}")
    return qf


def jpeg_compress(x, qf):
    """The round trip on the device: ``x`` CUDA [N,3,H,W], uint8 or float32 in [0,1] (quantised like ``eval.img_as_ubyte`` on the way in,
    converted like ``eval.img_as_float32`` on the way out) -> a new tensor of the same dtype and shape; per sample bit for bit
    ``eval.jpeg_compress`` of that image.

    ``qf``: one int for the whole batch, a sequence of N ints, or an int32 CUDA tensor [N] (no host-to-device copy, capturable once the
    device is warm); 1..100 is a quality, 0 returns that sample as it came (float values are not quantised).  The entries of a tensor are
    not read on the host: there, values above 100 count as 100 and negative ones as 0.  Not differentiable: the input is detached."""
    import torch
    from . import _native
    qf = _check_args(x, qf)
    src = x.detach().contiguous()
    n, _, h, w = src.shape
    with torch.cuda.device(src.device):
        if isinstance(qf, int):
            q = torch.empty(n, dtype=torch.int32, device=src.device).fill_(qf)
        elif isinstance(qf, list):
            q = torch.empty(n, dtype=torch.int32, device=src.device)
            q.copy_(torch.from_numpy(np.asarray(qf, dtype=np.int32)))
        else:
            q = qf.contiguous()
        tables = _device_tables(str(src.device))
        lib = _native.load()
        ws = torch.empty(lib.virnet_jpeg_workspace_bytes(n, h, w), dtype=torch.uint8, device=src.device)
        out = torch.empty(src.shape, dtype=src.dtype, device=src.device)
        f32 = int(src.dtype == torch.float32)
        _native.check(lib.virnet_jpeg_roundtrip(src.data_ptr(), f32, out.data_ptr(), f32, q.data_ptr(), tables.data_ptr(), ws.data_ptr(), n, h, w,
                                                _native.stream_handle()), "jpeg_roundtrip")
    return out
