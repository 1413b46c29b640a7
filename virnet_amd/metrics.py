"""uint8 PSNR / SSIM on the device (csrc/metrics.hip): the evaluation tables' metrics without a host round trip.

The definition is ``virnet_amd.eval`` (img_as_ubyte, rgb2y_uint8, calculate_psnr, calculate_ssim -- the reference's
utils/util_image.py:17-89,129-153 restated); this module gives the same numbers from CUDA tensors:

  * quantisation and the integer squared-error sum are exact, and PSNR is formed by the host's own double expression from them, so it
    is the same double;
  * SSIM is fp64 throughout and differs from the host only in summation order (separable filter, tiled sums): <= 1e-10;
  * luma is the fused chain ``fma(b, c2, fma(g, c1, r*c0)) + 16`` -- equal to ``eval.rgb2y_uint8`` except, on a host whose BLAS rounds the
    dot product the other way, on some of the 194 RGB triples whose exact luma ends in .5;
  * ``ycbcr="float"`` is the training scripts' test-stage metric instead (``util_image.batch_PSNR / batch_SSIM(..., ycbcr=True)``): the Y
    channel of the FLOAT image in fp32, every operation rounded on its own, quantised afterwards (:func:`rgb2y_float_np`).

Results are bitwise reproducible from run to run and do not depend on the batch an image sits in.  Nothing here synchronises: the calls
enqueue on the current stream of the tensors' device and return device tensors.  Not differentiable (inputs are detached).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _native

WINDOW, SIGMA = 11, 1.5


def gauss_taps() -> np.ndarray:
    """The 11 normalised 1-D window weights; ``eval._gauss_window()`` is their outer product."""
    g = np.exp(-((np.arange(WINDOW) - (WINDOW - 1) / 2.0) ** 2) / (2 * SIGMA ** 2))
    return g / g.sum()


_TAPS = (C.c_double * WINDOW)(*gauss_taps())


def _check(x: Tensor, name: str, dtypes) -> None:
    if not isinstance(x, Tensor) or x.dim() != 4:
        raise ValueError(f"{name} must be [N,C,H,W], got {tuple(getattr(x, 'shape', ()))}")
    if x.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {x.dtype}")


def _on_device(x: Tensor, name: str) -> Tensor:
    if not x.is_cuda:
        raise RuntimeError(f"{name} is on {x.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    return x.detach().contiguous()


def to_uint8(x: Tensor) -> Tensor:
    """float32 in the networks' [0,1] scale -> uint8, bit for bit ``eval.img_as_ubyte`` (values outside [0,1] are clamped first, as
    the tables clip before they quantise; NaN gives 0, where the host result is undefined)."""
    if not isinstance(x, Tensor) or x.dtype != torch.float32:
        raise TypeError(f"x must be a float32 tensor, got {getattr(x, 'dtype', type(x))}")
    x = _on_device(x, "x")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if x.numel():
        with torch.cuda.device(x.device):
            _native.check(_native.load().virnet_quantize_u8(x.data_ptr(), out.data_ptr(), x.numel(), _native.stream_handle()), "quantize_u8")
    return out


def rgb2y(u8: Tensor) -> Tensor:
    """uint8 RGB [N,3,H,W] -> uint8 Y [N,1,H,W] (``eval.rgb2y_uint8``)."""
    _check(u8, "u8", (torch.uint8,))
    if u8.shape[1] != 3:
        raise ValueError(f"u8 has {u8.shape[1]} channels, RGB expected")
    u8 = _on_device(u8, "u8")
    n, _, h, w = u8.shape
    out = torch.empty((n, 1, h, w), dtype=torch.uint8, device=u8.device)
    if out.numel():
        with torch.cuda.device(u8.device):
            _native.check(_native.load().virnet_rgb2y_u8(u8.data_ptr(), out.data_ptr(), n, h, w, _native.stream_handle()), "rgb2y_u8")
    return out


def rgb2y_float_np(x: np.ndarray) -> np.ndarray:
    """The definition of ``psnr_ssim(..., ycbcr="float")``'s luma: float32 RGB [N,3,H,W] -> float32 Y [N,1,H,W] in [0,1], the reference's
    ``util_image.rgb2ycbcrTorch(im, only_y=True)`` (:155-176) as a sequential fp32 chain -- every product, sum and the division rounded
    to float32 on its own: ``t = x*255``, ``k = fp32(coef)/255``, ``y = clip((((t_r*k_r + t_g*k_g) + t_b*k_b) + 16) / 255, 0, 1)``.
    ``eval.img_as_ubyte`` of it gives the bytes the test stage of the training scripts compares."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 4 or x.shape[1] != 3:
        raise ValueError(f"x must be float32 [N,3,H,W], got {x.dtype} {x.shape}")
    f255 = np.float32(255.0)
    k = np.array([65.481, 128.553, 24.966], dtype=np.float32) / f255
    t = x * f255
    y = (t[:, 0] * k[0] + t[:, 1] * k[1]) + t[:, 2] * k[2]
    y = (y + np.float32(16.0)) / f255
    return np.clip(y, np.float32(0.0), np.float32(1.0))[:, None]


def _ycbcr_mode(ycbcr) -> int:
    """The C ABI's ``ycbcr``: 0 channels as they are, 1 the Y of the quantised RGB image, 2 (``"float"``) the quantised Y of the float one."""
    if isinstance(ycbcr, str):
        if ycbcr != "float":
            raise ValueError(f"ycbcr={ycbcr!r}: False, True or 'float' expected")
        return 2
    return int(bool(ycbcr))


def psnr_ssim(a: Tensor, b: Tensor, border: int = 0, ycbcr=False, with_ssim: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
    """Metrics of the image pairs ``a[i]``, ``b[i]``: [N,C,H,W] CUDA tensors, C 1 or 3, each uint8 or float32 in [0,1] (quantised as by
    :func:`to_uint8` while it is read); ``ycbcr`` compares the Y channels of RGB inputs; ``border`` pixels are cropped on every side.
    ``ycbcr=True`` quantises RGB first and forms an integer Y (the evaluation scripts); ``ycbcr="float"`` forms Y from the float32 image
    in fp32 and quantises afterwards (the training scripts' test stage; :func:`rgb2y_float_np`; uint8 inputs are refused).

    Returns device tensors ``(sse int64 [N], count int64 [N], ssim float64 [N])``: the exact sum of squared uint8 differences over the
    cropped region and metric channels, its element count, and ``eval.calculate_ssim`` per image (NaN without ``with_ssim``).
    :func:`to_floats` turns them into the host functions' numbers.  No synchronisation; safe inside a caller's graph capture."""
    _check(a, "a", (torch.uint8, torch.float32))
    _check(b, "b", (torch.uint8, torch.float32))
    if a.shape != b.shape:
        raise ValueError("Input images must have the same dimensions.")
    n, c, h, w = a.shape
    if c not in (1, 3):
        raise ValueError(f"images have {c} channels, 1 or 3 expected")
    mode = _ycbcr_mode(ycbcr)
    if mode and c != 3:
        raise ValueError(f"ycbcr needs RGB images, got {c} channel(s)")
    if mode == 2 and (a.dtype != torch.float32 or b.dtype != torch.float32):
        raise TypeError(f"ycbcr='float' takes float32 images, got {a.dtype} and {b.dtype}")
    border = int(border)
    if border < 0:
        raise ValueError(f"border {border} is negative")
    need = (WINDOW if with_ssim else 1) + 2 * border
    if h < need or w < need:
        raise ValueError(f"images of {h}x{w} cropped by border {border} are smaller than "
                         f"{'the 11x11 SSIM window' if with_ssim else 'one pixel'}")
    if n == 0:
        raise ValueError("empty batch")
    a, b = _on_device(a, "a"), _on_device(b, "b")
    if a.device != b.device:
        raise RuntimeError(f"a is on {a.device}, b on {b.device}")
    lib = _native.load()
    with torch.cuda.device(a.device):
        ws = torch.empty(lib.virnet_psnr_ssim_workspace_bytes(n, c, h, w, border, mode) // 8, dtype=torch.int64, device=a.device)
        sse = torch.empty(n, dtype=torch.int64, device=a.device)
        count = torch.empty(n, dtype=torch.int64, device=a.device)
        ssim = torch.empty(n, dtype=torch.float64, device=a.device)
        _native.check(lib.virnet_psnr_ssim(a.data_ptr(), int(a.dtype == torch.float32), b.data_ptr(), int(b.dtype == torch.float32),
                                           n, c, h, w, border, mode, int(with_ssim), _TAPS, ws.data_ptr(), sse.data_ptr(),
                                           count.data_ptr(), ssim.data_ptr(), _native.stream_handle()), "psnr_ssim")
    return sse, count, ssim


def psnr_from_sse(sse: int, count: int) -> float:
    """``eval.calculate_psnr``'s expression on the exact error sum: the same double."""
    mse = float(np.float64(int(sse)) / np.float64(int(count)))
    return float("inf") if mse == 0 else 20.0 * math.log10(255.0 / math.sqrt(mse))


def to_floats(sse: Tensor, count: Tensor, ssim: Tensor) -> Tuple[List[float], List[float]]:
    """(per-image PSNR, per-image SSIM) as Python floats.  This is the synchronisation point: three small copies to the host."""
    s, c, q = sse.cpu().tolist(), count.cpu().tolist(), ssim.cpu().tolist()
    return [psnr_from_sse(x, y) for x, y in zip(s, c)], [float(v) for v in q]


# ---- glue for the evaluation tables (eval.denoise_table / sisr_eval.sisr_table with device_metrics=True) --------------------------------
def table_pair(mu: Tensor, gt_hwc: np.ndarray, border: int, ycbcr: bool, with_ssim: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """One image of a table: ``mu`` = the network's un-clipped output, a CUDA tensor [1,3,H,W] or [3,H,W]; ``gt_hwc`` = the uint8 H x W x 3
    ground truth on the host, which goes to the device once.  Enqueues the metric launches and returns their device results."""
    if not isinstance(mu, Tensor):
        raise TypeError(f"device_metrics=True: forward must return a CUDA tensor, got {type(mu).__name__}")
    if mu.dim() == 3:
        mu = mu.unsqueeze(0)
    if not mu.is_cuda:
        raise RuntimeError(f"device_metrics=True: forward returned a tensor on {mu.device}; return the network's CUDA output")
    gt = torch.from_numpy(np.ascontiguousarray(gt_hwc.transpose(2, 0, 1)[np.newaxis])).to(mu.device, non_blocking=True)
    return psnr_ssim(mu, gt, border=border, ycbcr=ycbcr, with_ssim=with_ssim)


def table_collect(pending: List[Tuple[Tensor, Tensor, Tensor]], with_ssim: bool) -> Tuple[List[float], List[float]]:
    """The per-image PSNR and SSIM lists of one (dataset, case) from its :func:`table_pair` results: ONE synchronisation."""
    if not pending:
        return [], []
    psnrs, ssims = to_floats(*(torch.cat(col) for col in zip(*pending)))
    return psnrs, (ssims if with_ssim else [])
