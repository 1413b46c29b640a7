"""The denoising objective and its variance prior on the device (csrc/elbo.hip).

  * :func:`elbo_denoising` -- ``loss.elbo_denoising_simple`` (loss/ELBO_simple.py:23-53, called as in train_denoising_syn.py:172-176 and
    train_denoising_real.py:165-171) as one fused pass: the three means are accumulated in fp64 from fp32 per-element terms, the
    gradients w.r.t. ``mu`` and ``sigma_est`` come from one closed-form kernel that reads the upstream gradient on the device;
  * :func:`noise_estimate` -- ``util_denoising.noise_estimate_fun`` (utils/util_denoising.py:53-63, train_denoising_real.py:164): the
    Gaussian-window local mean of ``(im_noisy - im_gt)**2`` with reflect border, clamped from below.

CUDA fp32 tensors only, no fallback.  Nothing here synchronises: the calls enqueue on the current stream of the tensors' device, and
results are bitwise reproducible (no atomics).  Dense NCHW tensors -- what ``train.denoise_forward_train`` returns for ``mu`` and
``sigma`` -- are read in place; any other layout goes through ``.contiguous()``.  The first call for a window size (or for a Python-float
``alpha0``) uploads a few constants: warm a shape up before capturing it into a graph.
"""
from __future__ import annotations

import functools
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _native

MAX_WINDOW = 31
# grid constants of csrc/elbo.hip (kThreads, kMaxBlocks): a value / gradient launch has min(ceil(items / THREADS), MAX_BLOCKS) workgroups,
# items = N*H*W / 4 in the 16-byte form (H*W a multiple of four) and N*H*W otherwise; one workgroup of THREADS threads adds the partials
THREADS, MAX_BLOCKS = 256, 1024


# ---- constants uploaded once -----------------------------------------------------------------------------------------------------------
def gaussian_taps(k_size: int) -> np.ndarray:
    """The 1-D window of ``util_denoising.inverse_gamma_kernel`` (utils/util_denoising.py:24-40) in float64: what OpenCV documents for
    ``getGaussianKernel(k, sigma)`` with a positive sigma, ``exp(-(i - (k-1)/2)^2 / (2 sigma^2))`` normalised to sum 1, at the reference's
    ``sigma = 0.3 ((k-1)/2 - 1) + 0.8``.  The 2-D window is the outer product (its renormalisation there is a no-op up to rounding)."""
    k = int(k_size)
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    i = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return g / g.sum()


@functools.lru_cache(maxsize=64)
def _device_taps(k_size: int, device: str) -> Tensor:
    """The window on the device, built once per (k, device): no per-call host-to-device copy."""
    with _native.capture_lock:
        return torch.from_numpy(gaussian_taps(k_size)).to(torch.device(device))


@functools.lru_cache(maxsize=64)
def _device_scalars(alpha0: float, device: str) -> Tensor:
    """[alpha0, digamma(alpha0 - 1)] in fp32 on the device for a Python-float alpha0 (the digamma on the host), once per value."""
    a = torch.tensor([alpha0], dtype=torch.float32)
    with _native.capture_lock:
        return torch.cat([a, torch.digamma(a - 1)]).to(torch.device(device))


def _scalars(alpha0, device: torch.device) -> Tensor:
    """fp32 [2] on ``device``: alpha0 and digamma(alpha0 - 1), without a host sync."""
    if not isinstance(alpha0, Tensor):
        return _device_scalars(float(alpha0), str(device))
    a = alpha0.detach().reshape(1)
    sc = torch.empty(2, dtype=torch.float32, device=device)
    sc[0:1].copy_(a)
    torch.digamma(a - 1, out=sc[1:2])
    return sc


# ---- argument checks (all before any device work) -----------------------------------------------------------------------------------------
def _check_images(named) -> None:
    for name, t in named:
        if not isinstance(t, Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() != 4:
            raise ValueError(f"{name} must be 4-D, got {tuple(t.shape)}")


def _check_devices(named) -> None:
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    first_name, first = named[0]
    for name, t in named[1:]:
        if t.device != first.device:
            raise RuntimeError(f"{first_name} is on {first.device}, {name} on {t.device}")


def _check_elbo_args(mus: Sequence[Tensor], sigma_est, im_noisy, im_gt, eps2, alpha0, beta0) -> None:
    named = [(f"mu[{i}]" if len(mus) > 1 else "mu", m) for i, m in enumerate(mus)]
    named += [("sigma_est", sigma_est), ("im_noisy", im_noisy), ("im_gt", im_gt), ("beta0", beta0)]
    _check_images(named)
    n, c, h, w = im_noisy.shape
    if n == 0 or c == 0 or h == 0 or w == 0:
        raise ValueError(f"im_noisy {tuple(im_noisy.shape)} is empty")
    for name, t in named:
        if name in ("sigma_est", "beta0"):
            if t.shape[0] != n or tuple(t.shape[2:]) != (h, w) or t.shape[1] not in (1, c):
                raise ValueError(f"{name} must be [{n},1,{h},{w}] or [{n},{c},{h},{w}], got {tuple(t.shape)}")
        elif tuple(t.shape) != (n, c, h, w):
            raise ValueError(f"{name} {tuple(t.shape)} != im_noisy {(n, c, h, w)}")
    if n * h * w >= 1 << 31 or h > 32768 or w > 32768:
        raise ValueError(f"{n} images of {h}x{w}: n*h*w must stay below 2^31 and h, w at most 32768")
    if isinstance(eps2, (bool, Tensor)) or not float(eps2) > 0.0:
        raise ValueError(f"eps2 {eps2!r}: a positive float is expected")
    if isinstance(alpha0, Tensor):
        if alpha0.numel() != 1 or alpha0.dtype != torch.float32:
            raise TypeError(f"alpha0 must be a float or a one-element float32 tensor, got {tuple(alpha0.shape)} {alpha0.dtype}")
        named = named + [("alpha0", alpha0)]
    elif isinstance(alpha0, bool) or not isinstance(alpha0, (int, float)):
        raise TypeError(f"alpha0 must be a float or a one-element float32 tensor, got {type(alpha0).__name__}")
    elif not float(alpha0) > 1.0:
        raise ValueError(f"alpha0 {alpha0!r}: the prior's shape alpha0 - 1 must be positive")
    _check_devices(named)


# ---- launches (inputs contiguous fp32 on one device; the caller holds torch.cuda.device) --------------------------------------------------
def _value(mu: Tensor, sig: Tensor, x: Tensor, gt: Tensor, b0: Tensor, sc: Tensor, eps2: float, with_klig: bool) -> Tensor:
    n, c, h, w = x.shape
    lib = _native.load()
    ws = torch.empty(lib.virnet_elbo_workspace_bytes(n, c, h, w) // 8, dtype=torch.float64, device=x.device)
    out = torch.empty(4, dtype=torch.float32, device=x.device)
    _native.check(lib.virnet_elbo_value(mu.data_ptr(), sig.data_ptr(), x.data_ptr(), gt.data_ptr(), b0.data_ptr(), sc.data_ptr(), sc.data_ptr() + 4,
                                        eps2, int(with_klig), ws.data_ptr(), out.data_ptr(), n, c, sig.shape[1], b0.shape[1], h, w,
                                        _native.stream_handle()), "elbo_value")
    return out


def _grad(mu: Tensor, sig: Tensor, x: Tensor, gt: Tensor, b0: Tensor, sc: Tensor, g: Tensor, eps2: float, w_data: float,
          w_klig: float) -> Tuple[Tensor, Tensor]:
    n, c, h, w = x.shape
    dmu = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    dsig = torch.empty(tuple(sig.shape), dtype=torch.float32, device=x.device)
    _native.check(_native.load().virnet_elbo_grad(mu.data_ptr(), sig.data_ptr(), x.data_ptr(), gt.data_ptr(), b0.data_ptr(), sc.data_ptr(), g.data_ptr(),
                                                  eps2, w_data, w_klig, dmu.data_ptr(), dsig.data_ptr(), n, c, sig.shape[1], b0.shape[1], h, w,
                                                  _native.stream_handle()), "elbo_grad")
    return dmu, dsig


class _ElboDenoising(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sigma_est: Tensor, im_noisy: Tensor, im_gt: Tensor, beta0: Tensor, sc: Tensor, eps2: float, *mus: Tensor):
        sig, x, gt, b0 = (t.detach().contiguous() for t in (sigma_est, im_noisy, im_gt, beta0))
        ms = [m.detach().contiguous() for m in mus]
        with torch.cuda.device(x.device):
            outs = [_value(m, sig, x, gt, b0, sc, eps2, i == 0) for i, m in enumerate(ms)]      # the variance term once, with the first
            if len(outs) == 1:
                loss, lh, klg, klig = outs[0].unbind(0)
            else:
                klig = outs[0][3]
                lh, klg = outs[0][1], outs[0][2]
                for o in outs[1:]:
                    lh, klg = lh + o[1], klg + o[2]
                lh, klg = lh / len(outs), klg / len(outs)
                loss = lh + klg + klig
        ctx.eps2 = eps2
        ctx.save_for_backward(sig, x, gt, b0, sc, *ms)
        ctx.mark_non_differentiable(lh, klg, klig)
        return loss, lh, klg, klig

    @staticmethod
    def backward(ctx, g_loss: Tensor, *_unused):
        if torch.is_grad_enabled():
            raise RuntimeError("elbo.elbo_denoising: double backward (create_graph=True) is not supported -- the backward runs on a HIP "
                               "kernel outside autograd and is first-order only")
        sig, x, gt, b0, sc, *ms = ctx.saved_tensors
        need_sig, need_mu = ctx.needs_input_grad[0], ctx.needs_input_grad[6:]
        dsig, dmus = None, [None] * len(ms)
        with torch.cuda.device(x.device):
            g = g_loss.detach()
            if g.dtype != torch.float32:
                g = g.float()
            g = g.contiguous()
            for i, m in enumerate(ms):
                if not (need_sig or need_mu[i]):
                    continue
                dm, ds = _grad(m, sig, x, gt, b0, sc, g, ctx.eps2, 1.0 / len(ms), 1.0 if i == 0 else 0.0)
                dmus[i] = dm if need_mu[i] else None
                dsig = ds if dsig is None else dsig.add_(ds)
        return (dsig if need_sig else None, None, None, None, None, None) + tuple(dmus)


def elbo_denoising(mu: Union[Tensor, Sequence[Tensor]], sigma_est: Tensor, im_noisy: Tensor, im_gt: Tensor, eps2: float, alpha0,
                   beta0: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(loss, lh, kl_gauss, kl_Igamma)`` of ``loss.elbo_denoising_simple`` as 0-dim CUDA tensors.

    ``mu``, ``im_noisy``, ``im_gt``: [N,C,H,W] fp32; ``sigma_est`` [N,Cs,H,W] and ``beta0`` [N,Cb,H,W] with Cs, Cb each 1 or C, broadcast as
    the torch expressions broadcast them (``kl_Igamma`` averages over N max(Cs,Cb) H W elements).  ``alpha0``: a one-element fp32 tensor on
    the same device (its digamma is taken on the device, no sync) or a Python float.  ``mu`` may be a list or tuple of restorer outputs
    (deep supervision, ELBO_simple.py:30-34,43-47): one value / gradient launch per entry, ``lh`` and ``kl_gauss`` averaged over the
    entries, the variance term computed once.

    ``loss`` is differentiable (first order) in ``mu`` and ``sigma_est``.  ``lh``, ``kl_gauss`` and ``kl_Igamma`` are marked
    non-differentiable: the reference only logs them (train_denoising_syn.py:186-189).  ``im_noisy``, ``im_gt``, ``alpha0`` and ``beta0``
    are data and get no gradient."""
    mus: List[Tensor] = list(mu) if isinstance(mu, (list, tuple)) else [mu]
    if not mus:
        raise ValueError("elbo_denoising: empty list of restorer outputs")
    _check_elbo_args(mus, sigma_est, im_noisy, im_gt, eps2, alpha0, beta0)
    with torch.no_grad(), torch.cuda.device(im_noisy.device):
        sc = _scalars(alpha0, im_noisy.device)
    return _ElboDenoising.apply(sigma_est, im_noisy, im_gt, beta0, sc, float(eps2), *mus)


def noise_estimate(im_noisy: Tensor, im_gt: Tensor, k_size: int, floor: float = 1e-10) -> Tensor:
    """``max(G_k (*) (im_noisy - im_gt)**2, floor)``: [N,C,H,W] fp32 -> [N,C,H,W] fp32, the variance prior ``noise_estimate_fun`` of
    utils/util_denoising.py:53-63 (Gaussian window :func:`gaussian_taps`, reflect border).  ``k_size`` odd, 1..31, k_size // 2 < min(H, W).
    The squared error never exists in memory; the window runs separably in fp64.  Not differentiable (the inputs are data)."""
    _check_images([("im_noisy", im_noisy), ("im_gt", im_gt)])
    if im_noisy.shape != im_gt.shape:
        raise ValueError(f"im_gt {tuple(im_gt.shape)} != im_noisy {tuple(im_noisy.shape)}")
    if isinstance(k_size, bool) or int(k_size) != k_size or int(k_size) % 2 == 0 or not 1 <= int(k_size) <= MAX_WINDOW:
        raise ValueError(f"window size {k_size!r}: odd sizes 1..{MAX_WINDOW} are supported")
    k = int(k_size)
    n, c, h, w = im_noisy.shape
    if n == 0 or c == 0 or n * c > 65535:
        raise ValueError(f"batch x channels = {n} x {c} outside 1..65535")
    if h > 32768 or w > 32768:
        raise ValueError(f"image {h}x{w} is larger than 32768")
    if k // 2 >= min(h, w):
        raise ValueError(f"padding {k // 2} of a {k}x{k} window must be smaller than the image ({h}x{w})")
    _check_devices([("im_noisy", im_noisy), ("im_gt", im_gt)])
    with torch.no_grad(), torch.cuda.device(im_noisy.device):
        x, gt = im_noisy.detach().contiguous(), im_gt.detach().contiguous()
        taps = _device_taps(k, str(x.device))
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        _native.check(_native.load().virnet_noise_estimate(x.data_ptr(), gt.data_ptr(), taps.data_ptr(), out.data_ptr(), n, c, h, w, k, float(floor),
                                                           _native.stream_handle()), "noise_estimate")
    return out
