"""The SISR degradation ``y = D_sf(k_n (*) x_n)`` on the device (csrc/degrade.hip), with its adjoints.

The operator reflect-pads the HR image, correlates it with one k x k kernel per sample (shared by the channels) and keeps every sf-th
sample ("direct") or applies the antialiased cubic resize ("bicubic").  Its definitions on the host are ``loss.blur_downsample``
(utils/util_sisr.py:127-144, the training likelihood of loss/ELBO_simple.py:55-59) and ``sisr_eval.degrade`` (utils/util_sisr.py:146-166,
the synthetic evaluation input); this module computes the same from CUDA tensors on the project's own kernels:

  * :func:`blur_downsample` -- differentiable in the image and in the kernel (first order), e.g. as the data term of a plug-and-play
    objective ``|| y - D(k (*) x) ||^2`` next to the frozen network's input-image gradients;
  * :func:`degrade_lr`      -- ``sisr_eval.degrade`` for one ground-truth image: blur, clip, downsample on the device; the seeded float64
    noise is still drawn on the host, so the stream is the reference's; with ``qf`` the JPEG round trip (virnet_amd/jpeg.py) ends it;
  * :func:`synthesize_lr`   -- the tail of the training dataset (datasets/SISRDatasets.py:89-112) for a batch that is already on the device:
    blur, clip, downsample, the caller's noise, clip, JPEG round trip with one quality per sample.

fp32 vector arithmetic for the blur (error: a few ulps of sum |k||x|), fp64 for the resize taps.  Results are bitwise reproducible and
do not depend on the batch an image sits in.  Nothing here synchronises: the calls enqueue on the current stream of the tensors' device.
The first call for an image size builds the resize tap tables on the host and uploads them (once per size, factor and device): warm a
shape up before capturing it into a graph.
"""
from __future__ import annotations

import functools
import math
from typing import Tuple

import numpy as np
import torch
from torch import Tensor

from . import _native, sisr_eval

MAX_KERNEL, MAX_SF = 25, 4
BORDERS = {"reflect": _native.BORDER_REFLECT, "symmetric": _native.BORDER_SYMMETRIC}


# ---- tap tables of the antialiased cubic --------------------------------------------------------------------------------------------------
def tap_table(n_in: int, sf: int) -> Tuple[np.ndarray, np.ndarray]:
    """(idx int32, wgt float64), both [ceil(n_in/sf), taps]: ``out[o] = sum_t wgt[o, t] * in[idx[o, t]]`` (sisr_eval.resample_taps)."""
    scale = 1.0 / sf
    idx, wgt = sisr_eval.resample_taps(int(n_in), scale, math.ceil(scale * n_in))
    return np.ascontiguousarray(idx.astype(np.int32)), np.ascontiguousarray(wgt)


def transpose_taps(idx: np.ndarray, wgt: np.ndarray, n_in: int) -> Tuple[np.ndarray, np.ndarray]:
    """The table of the transposed (adjoint) map, [n_in, longest row]: row a lists the (o, weight) pairs of the taps that read input a, in
    the order (o, t); shorter rows are padded with zero weights."""
    n_out, taps = idx.shape
    rows = [[] for _ in range(n_in)]
    for o in range(n_out):
        for t in range(taps):
            rows[int(idx[o, t])].append((o, float(wgt[o, t])))
    width = max(1, max(len(r) for r in rows))
    idx_t = np.zeros((n_in, width), dtype=np.int32)
    wgt_t = np.zeros((n_in, width), dtype=np.float64)
    for a, r in enumerate(rows):
        for s, (o, v) in enumerate(r):
            idx_t[a, s], wgt_t[a, s] = o, v
    return idx_t, wgt_t


def densify(idx: np.ndarray, wgt: np.ndarray, n_cols: int) -> np.ndarray:
    """[rows, n_cols] float64 matrix of a tap table."""
    mat = np.zeros((idx.shape[0], n_cols))
    np.add.at(mat, (np.repeat(np.arange(idx.shape[0]), idx.shape[1]), idx.reshape(-1)), wgt.reshape(-1))
    return mat


@functools.lru_cache(maxsize=64)
def _device_taps(n_in: int, sf: int, device: str):
    """(idx, wgt, idx_t, wgt_t) on the device, built once per (size, factor, device): no per-call host-to-device copy."""
    idx, wgt = tap_table(n_in, sf)
    idx_t, wgt_t = transpose_taps(idx, wgt, n_in)
    dev = torch.device(device)
    with _native.capture_lock:
        return tuple(torch.from_numpy(a).to(dev) for a in (idx, wgt, idx_t, wgt_t))


def warm_taps(h: int, w: int, sf: int, device) -> None:
    """Build and upload the bicubic tap tables of an h x w image ahead of time (before a graph capture, or outside a timed region)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    _device_taps(int(h), int(sf), str(dev))
    _device_taps(int(w), int(sf), str(dev))


# ---- argument checks (all before any device work) -----------------------------------------------------------------------------------------
def _check_args(im_hr, kernel, sf, downsampler, border) -> Tuple[int, int, int]:
    for name, t in (("im_hr", im_hr), ("kernel", kernel)):
        if not isinstance(t, Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() != 4:
            raise ValueError(f"{name} must be 4-D, got {tuple(t.shape)}")
    n, c, h, w = im_hr.shape
    if kernel.shape[1] != 1 or kernel.shape[2] != kernel.shape[3]:
        raise ValueError(f"kernel must be [N,1,k,k], got {tuple(kernel.shape)}")
    if kernel.shape[0] != n:
        raise ValueError(f"kernel batch {kernel.shape[0]} != image batch {n}: one kernel per sample")
    k = int(kernel.shape[-1])
    if k % 2 == 0 or not 1 <= k <= MAX_KERNEL:
        raise ValueError(f"kernel size {k}: odd sizes 1..{MAX_KERNEL} are supported")
    if isinstance(sf, bool) or int(sf) != sf or not 1 <= int(sf) <= MAX_SF:
        raise ValueError(f"sf {sf!r}: integer scale factors 1..{MAX_SF} are supported")
    if n == 0 or c == 0 or n * c > 65535:
        raise ValueError(f"batch x channels = {n} x {c} outside 1..65535")
    if h > 32768 or w > 32768:
        raise ValueError(f"image {h}x{w} is larger than 32768")
    if k // 2 >= min(h, w):
        raise ValueError(f"padding {k // 2} of a {k}x{k} kernel must be smaller than the image ({h}x{w})")
    mode = str(downsampler).lower()
    if mode not in ("direct", "bicubic"):
        raise ValueError("downsampler must be 'direct' or 'bicubic'")
    if border not in BORDERS:
        raise ValueError(f"border must be one of {sorted(BORDERS)}, got {border!r}")
    for name, t in (("im_hr", im_hr), ("kernel", kernel)):
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    if im_hr.device != kernel.device:
        raise RuntimeError(f"im_hr is on {im_hr.device}, kernel on {kernel.device}")
    return k, int(sf), BORDERS[border]


# ---- launches (inputs contiguous fp32 on one device; the caller holds torch.cuda.device) --------------------------------------------------
def _blur(x: Tensor, kernel: Tensor, sf: int, border: int, clip: bool) -> Tensor:
    n, c, h, w = x.shape
    y = torch.empty((n, c, -(-h // sf), -(-w // sf)), dtype=torch.float32, device=x.device)
    _native.check(_native.load().virnet_degrade_forward(x.data_ptr(), kernel.data_ptr(), y.data_ptr(), n, c, h, w, kernel.shape[-1], sf, border,
                                                        int(clip), _native.stream_handle()), "degrade_forward")
    return y


def _blur_grad_image(gy: Tensor, kernel: Tensor, shape, sf: int, border: int) -> Tensor:
    n, c, h, w = shape
    gx = torch.empty(shape, dtype=torch.float32, device=gy.device)
    _native.check(_native.load().virnet_degrade_grad_image(gy.data_ptr(), kernel.data_ptr(), gx.data_ptr(), n, c, h, w, kernel.shape[-1], sf, border,
                                                           _native.stream_handle()), "degrade_grad_image")
    return gx


def _blur_grad_kernel(gy: Tensor, x: Tensor, k: int, sf: int, border: int) -> Tensor:
    n, c, h, w = x.shape
    lib = _native.load()
    ws = torch.empty(lib.virnet_degrade_grad_kernel_workspace_bytes(n, c, h, w, k, sf) // 4, dtype=torch.float32, device=x.device)
    gk = torch.empty((n, 1, k, k), dtype=torch.float32, device=x.device)
    _native.check(lib.virnet_degrade_grad_kernel(gy.data_ptr(), x.data_ptr(), gk.data_ptr(), ws.data_ptr(), n, c, h, w, k, sf, border,
                                                 _native.stream_handle()), "degrade_grad_kernel")
    return gk


def _resample(src: Tensor, idx: Tensor, wgt: Tensor, axis: int, n_out: int) -> Tensor:
    """fp32 -> fp64 or fp64 -> fp32 along ``axis`` (2 or 3) of a contiguous NCHW tensor."""
    shape = list(src.shape)
    n_in = shape[axis]
    shape[axis] = n_out
    out = torch.empty(shape, dtype=torch.float32 if src.dtype == torch.float64 else torch.float64, device=src.device)
    outer = math.prod(shape[:axis])
    inner = math.prod(shape[axis + 1:])
    _native.check(_native.load().virnet_resample_axis(src.data_ptr(), int(src.dtype == torch.float64), out.data_ptr(), int(out.dtype == torch.float64),
                                                      idx.data_ptr(), wgt.data_ptr(), idx.shape[1], outer, n_in, n_out, inner,
                                                      _native.stream_handle()), "resample_axis")
    return out


class _BlurDownsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im_hr: Tensor, kernel: Tensor, sf: int, bicubic: bool, border: int, clip: bool) -> Tensor:
        x, ker = im_hr.detach().contiguous(), kernel.detach().contiguous()
        need_x, need_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.sf, ctx.bicubic, ctx.border, ctx.shape, ctx.k = sf, bicubic, border, tuple(x.shape), int(ker.shape[-1])
        ctx.save_for_backward(x if need_k else None, ker if need_x else None)
        with torch.cuda.device(x.device):
            if not bicubic:
                return _blur(x, ker, sf, border, clip)
            h, w = x.shape[-2:]
            th, tw = _device_taps(h, sf, str(x.device)), _device_taps(w, sf, str(x.device))
            blur = _blur(x, ker, 1, border, clip)
            rows = _resample(blur, th[0], th[1], 2, th[0].shape[0])                 # fp64 [N,C,h/sf,W]
            return _resample(rows, tw[0], tw[1], 3, tw[0].shape[0])                # fp32 [N,C,h/sf,w/sf]

    @staticmethod
    def backward(ctx, gy: Tensor):
        if torch.is_grad_enabled():
            raise RuntimeError("degrade.blur_downsample: double backward (create_graph=True) is not supported -- the backward runs on HIP "
                               "kernels outside autograd and is first-order only")
        x, ker = ctx.saved_tensors
        need_x, need_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        n, c, h, w = ctx.shape
        sf = ctx.sf
        with torch.cuda.device(gy.device):
            g = gy.detach()
            if g.dtype != torch.float32:
                g = g.float()
            g = g.contiguous()
            if ctx.bicubic:
                th, tw = _device_taps(h, sf, str(g.device)), _device_taps(w, sf, str(g.device))
                cols = _resample(g, tw[2], tw[3], 3, w)                             # fp64 [N,C,h/sf,W]
                g = _resample(cols, th[2], th[3], 2, h)                            # fp32 [N,C,H,W]
                sf = 1
            gx = _blur_grad_image(g, ker, ctx.shape, sf, ctx.border) if need_x else None
            gk = _blur_grad_kernel(g, x, ctx.k, sf, ctx.border) if need_k else None
        return gx, gk, None, None, None, None


def blur_downsample(im_hr: Tensor, kernel: Tensor, sf: int, downsampler: str = "direct", border: str = "reflect", clip: bool = False) -> Tensor:
    """``D_sf(kernel_n (*) im_hr_n)``: [N,C,H,W] fp32, [N,1,k,k] fp32 (k odd, <= 25; cross-correlation, one kernel per sample) ->
    [N,C,ceil(H/sf),ceil(W/sf)] fp32, sf 1..4.

    ``downsampler``: "direct" keeps every sf-th sample of the blur (only those are computed), "bicubic" resizes the blur by the
    antialiased cubic.  ``border``: "reflect" (``d c b | a b c d``, the training operator ``loss.blur_downsample``) or "symmetric"
    (``c b a | a b c``, scipy's "reflect", the evaluation operator ``sisr_eval.degrade``); k // 2 < min(H, W) either way.  ``clip`` clamps the
    blur to [0, 1] before the downsampling, as the evaluation does; it is not differentiable here.

    Differentiable (first order) in ``im_hr`` and ``kernel``, each computed only when it requires a gradient."""
    k, sf, bmode = _check_args(im_hr, kernel, sf, downsampler, border)
    if clip and torch.is_grad_enabled() and (im_hr.requires_grad or kernel.requires_grad):
        raise RuntimeError("degrade.blur_downsample: clip=True is not differentiable; detach the inputs or pass clip=False")
    return _BlurDownsample.apply(im_hr, kernel, sf, str(downsampler).lower() == "bicubic", bmode, bool(clip))


def degrade_lr(im_hr: np.ndarray, kernel: np.ndarray, sf: int, nlevel: float = 2.55, seed: int = sisr_eval.NOISE_SEED, downsampler: str = "bicubic",
               device=None, qf=None) -> Tensor:
    """``sisr_eval.degrade`` with the blur, clip and downsampling on the device: fp32 [h,w,3] image in [0,1] and [k,k] kernel on the host ->
    LR CUDA tensor [1,3,ceil(h/sf),ceil(w/sf)] fp32.  The kernel is flipped on the host (``ndimage.convolve`` is a true convolution), the
    border is "symmetric", the blur is clipped; the float64 noise is the host's seeded stream, uploaded at LR size, added in fp64, then
    cast and clipped as there.  ``qf``: JPEG quality of a final round trip on the device (``jpeg.jpeg_compress``), None for none."""
    if not isinstance(im_hr, np.ndarray) or im_hr.dtype != np.float32:
        raise TypeError("degrade_lr expects a float32 image in [0,1]")
    if im_hr.ndim != 3:
        raise ValueError(f"degrade_lr expects an [h,w,c] image, got {im_hr.shape}")
    mode = str(downsampler).lower()
    if mode not in ("direct", "bicubic"):
        raise ValueError("downsampler must be 'direct' or 'bicubic'")
    if qf is not None and (isinstance(qf, bool) or int(qf) != qf or not 1 <= int(qf) <= 100):
        raise ValueError(f"qf {qf!r}: None or a JPEG quality 1..100")
    if not torch.cuda.is_available():
        raise RuntimeError("degrade_lr: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    x = torch.from_numpy(np.ascontiguousarray(im_hr.transpose(2, 0, 1)[np.newaxis])).to(dev, non_blocking=True)
    ker = torch.from_numpy(np.ascontiguousarray(np.asarray(kernel, dtype=np.float64)[::-1, ::-1]).astype(np.float32)[np.newaxis, np.newaxis]).to(dev)
    with torch.no_grad():
        lr = blur_downsample(x, ker, sf, mode, border="symmetric", clip=True)
    hl, wl = lr.shape[-2:]
    noise = np.random.default_rng(seed).standard_normal(size=(hl, wl, im_hr.shape[2])) * (nlevel / 255.0)
    noise = torch.from_numpy(np.ascontiguousarray(noise.transpose(2, 0, 1)[np.newaxis])).to(dev, non_blocking=True)
    lr = (lr.double() + noise).float().clamp_(0.0, 1.0)
    if qf is not None:
        from . import jpeg
        lr = jpeg.jpeg_compress(lr, int(qf))
    return lr


def synthesize_lr(im_hr: Tensor, kernel: Tensor, sf: int, noise: Tensor, std: Tensor, qf=None, downsampler: str = "bicubic") -> Tuple[Tensor, Tensor]:
    """The tail of GeneralTrainFloder.__getitem__ (datasets/SISRDatasets.py:89-112) for a batch on the device -> (im_lr, im_blur), both
    [N,3,ceil(H/sf),ceil(W/sf)] fp32.  ``im_hr`` [N,3,H,W] fp32 in [0,1]; ``kernel`` [N,1,k,k] as the dataset makes it, i.e. applied as a
    true convolution (it is flipped here); ``noise`` standard normal of the LR shape, drawn by the caller so the random stream stays theirs;
    ``std`` fp32 [N], the noise level per sample; ``qf`` int32 [N] (or anything ``jpeg.jpeg_compress`` takes), 0 for a sample without
    JPEG, None for none at all.

    im_blur = ``blur_downsample(im_hr, flipped kernel, sf, downsampler, border="symmetric", clip=True)``;
    im_lr = ``clip(im_blur + noise * std, 0, 1)`` in fp32 with the product and the sum rounded separately, then the round trip.
    The host counterpart is ``sisr_eval.synthesize_lr_np``.  Not differentiable."""
    for name, t in (("noise", noise), ("std", std)):
        if not isinstance(t, Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    if not isinstance(im_hr, Tensor) or not isinstance(kernel, Tensor):
        raise TypeError("im_hr and kernel must be tensors")
    if im_hr.dim() != 4 or im_hr.shape[1] != 3:
        raise ValueError(f"im_hr must be [N,3,H,W], got {tuple(im_hr.shape)}")
    n, _, h, w = im_hr.shape
    if isinstance(sf, bool) or int(sf) != sf or not 1 <= int(sf) <= MAX_SF:
        raise ValueError(f"sf {sf!r}: integer scale factors 1..{MAX_SF} are supported")
    lr_shape = (n, 3, -(-h // int(sf)), -(-w // int(sf)))
    if tuple(noise.shape) != lr_shape:
        raise ValueError(f"noise must have the LR shape {lr_shape}, got {tuple(noise.shape)}")
    if tuple(std.shape) != (n,):
        raise ValueError(f"std must be [{n}], one level per sample, got {tuple(std.shape)}")
    with torch.no_grad():
        im_blur = blur_downsample(im_hr.detach(), kernel.detach().flip(-2, -1), sf, downsampler, border="symmetric", clip=True)
        for name, t in (("noise", noise), ("std", std)):
            if t.device != im_blur.device:
                raise RuntimeError(f"im_hr is on {im_blur.device}, {name} on {t.device}")
        im_lr = (im_blur + noise * std.view(n, 1, 1, 1)).clamp_(0.0, 1.0)
        if qf is not None:
            from . import jpeg
            im_lr = jpeg.jpeg_compress(im_lr, qf)
    return im_lr, im_blur
