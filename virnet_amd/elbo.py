"""The training objectives and the denoising variance prior on the device (csrc/elbo.hip, csrc/elbo_sisr.hip).

  * :func:`elbo_denoising` -- ``loss.elbo_denoising_simple`` (loss/ELBO_simple.py:23-53, called as in train_denoising_syn.py:172-176 and
    train_denoising_real.py:165-171) as one fused pass: the three means are accumulated in fp64 from fp32 per-element terms, the
    gradients w.r.t. ``mu`` and ``sigma_est`` come from one closed-form kernel that reads the upstream gradient on the device;
  * :func:`noise_estimate` -- ``util_denoising.noise_estimate_fun`` (utils/util_denoising.py:53-63, train_denoising_real.py:164): the
    Gaussian-window local mean of ``(im_noisy - im_gt)**2`` with reflect border, clamped from below;
  * :func:`elbo_sisr` -- ``loss.elbo_sisr`` (loss/ELBO_simple.py:55-138 with the kernel of utils/util_sisr.py:26-58, called as in
    train_SISR.py:207-224): the KernelNet head, the HR pass and the LR pass around the degradation, each one value and one gradient kernel.

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
MAX_SISR_KERNEL, MAX_SISR_SF = 25, 4          # the degradation's limits (degrade.MAX_KERNEL, degrade.MAX_SF)
# grid constants of csrc/elbo.hip (kThreads, kMaxBlocks): a value / gradient launch has min(ceil(items / THREADS), MAX_BLOCKS) workgroups,
# items = N*H*W / 4 in the 16-byte form (H*W a multiple of four) and N*H*W otherwise; one workgroup of THREADS threads adds the partials
THREADS, MAX_BLOCKS = 256, 1024
# grid constants of csrc/elbo_sisr.hip (kThreads, kMaxBlocks, kLrBlocks): an HR launch has min(ceil(items / SISR_THREADS), SISR_MAX_BLOCKS)
# workgroups, items = N*C*H*W / 4 in the 16-byte form (H*W a multiple of four) and N*C*H*W otherwise; an LR launch has, per sample,
# min(ceil(items / SISR_THREADS), SISR_LR_BLOCKS) workgroups, items = h*w / 4 or h*w; one workgroup of SISR_THREADS threads adds the partials
SISR_THREADS, SISR_MAX_BLOCKS, SISR_LR_BLOCKS = 256, 1024, 256


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


# ---- SISR objective (csrc/elbo_sisr.hip) -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _device_float(value: float, device: str) -> Tensor:
    """One fp32 scalar on the device for a Python-float constant (kappa0), once per value."""
    with _native.capture_lock:
        return torch.tensor([value], dtype=torch.float32).to(torch.device(device))


def _check_shape_scalar(name: str, v, named: list) -> None:
    """alpha0 / kappa0: a one-element fp32 tensor (appended to ``named`` for the device check) or a Python float above 1"""
    if isinstance(v, Tensor):
        if v.numel() != 1 or v.dtype != torch.float32:
            raise TypeError(f"{name} must be a float or a one-element float32 tensor, got {tuple(v.shape)} {v.dtype}")
        named.append((name, v))
    elif isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be a float or a one-element float32 tensor, got {type(v).__name__}")
    elif not float(v) > 1.0:
        raise ValueError(f"{name} {v!r}: the prior's shape {name} - 1 must be positive")


def _positive_float(name: str, v) -> None:
    if isinstance(v, (bool, Tensor)) or not isinstance(v, (int, float)) or not float(v) > 0.0 or float(v) == float("inf"):
        raise ValueError(f"{name} {v!r}: a positive float is expected")


def _check_sisr_args(mu, sigma_est, kinfo_est, im_hr, im_lr, sigma_prior, alpha0, kinfo_gt, kappa0, r2, eps2, sf, k_size, penalty_K, downsampler,
                     degrade_impl, draws) -> None:
    named = [("mu", mu), ("sigma_est", sigma_est), ("im_hr", im_hr), ("im_lr", im_lr), ("sigma_prior", sigma_prior)]
    _check_images(named)
    for name, t in (("kinfo_est", kinfo_est), ("kinfo_gt", kinfo_gt)):
        if not isinstance(t, Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        named.append((name, t))
    n, c, h, w = mu.shape
    if n == 0 or c == 0 or h == 0 or w == 0:
        raise ValueError(f"mu {tuple(mu.shape)} is empty")
    if tuple(im_hr.shape) != (n, c, h, w):
        raise ValueError(f"im_hr {tuple(im_hr.shape)} != mu {(n, c, h, w)}")
    for name, t in (("kinfo_est", kinfo_est), ("kinfo_gt", kinfo_gt)):
        if tuple(t.shape) != (n, 3):
            raise ValueError(f"{name} must be [{n},3], got {tuple(t.shape)}")
    if degrade_impl not in ("hip", "torch"):
        raise ValueError("degrade_impl must be 'hip' or 'torch'")
    if isinstance(sf, bool) or not isinstance(sf, int) or not 1 <= sf <= MAX_SISR_SF:
        raise ValueError(f"sf {sf!r}: integer scale factors 1..{MAX_SISR_SF} are supported")
    if isinstance(k_size, bool) or not isinstance(k_size, int) or not 1 <= k_size <= MAX_SISR_KERNEL:
        raise ValueError(f"k_size {k_size!r}: kernel sizes 1..{MAX_SISR_KERNEL} are supported")
    if degrade_impl == "hip" and k_size % 2 == 0:
        raise ValueError(f"k_size {k_size}: the device degradation takes odd kernel sizes")
    if k_size // 2 >= min(h, w):
        raise ValueError(f"padding {k_size // 2} of a {k_size}x{k_size} kernel must be smaller than the image ({h}x{w})")
    if str(downsampler).lower() not in ("direct", "bicubic"):
        raise ValueError("downsampler must be 'direct' or 'bicubic'")
    if n > 65535 or n * c > 65535 or h > 32768 or w > 32768 or n * c * h * w >= 1 << 31:
        raise ValueError(f"{n} x {c} images of {h}x{w}: n*c at most 65535, h and w at most 32768, n*c*h*w below 2^31")
    hl, wl = -(-h // sf), -(-w // sf)
    if tuple(im_lr.shape) != (n, c, hl, wl):
        raise ValueError(f"im_lr {tuple(im_lr.shape)} != the degradation's output {(n, c, hl, wl)} for a {h}x{w} image, sf {sf}, {downsampler}")
    for name, t in (("sigma_est", sigma_est), ("sigma_prior", sigma_prior)):
        if tuple(t.shape) not in ((n, 1, 1, 1), (n, 1, hl, wl), (n, c, hl, wl)):
            raise ValueError(f"{name} must be [{n},1,1,1], [{n},1,{hl},{wl}] or [{n},{c},{hl},{wl}], got {tuple(t.shape)}")
    _positive_float("eps2", eps2)
    _positive_float("r2", r2)
    _check_shape_scalar("alpha0", alpha0, named)
    _check_shape_scalar("kappa0", kappa0, named)
    try:
        pen = [float(p) for p in penalty_K]
    except (TypeError, ValueError):
        raise TypeError(f"penalty_K {penalty_K!r}: two floats are expected") from None
    if len(pen) != 2 or any(isinstance(p, (bool, Tensor)) for p in penalty_K) or not all(np.isfinite(pen)):
        raise ValueError(f"penalty_K {penalty_K!r}: two finite floats are expected")
    if draws is not None:
        if not isinstance(draws, (tuple, list)) or len(draws) != 3:
            raise TypeError("draws must be None or (gamma [N,2], rho_eps [N,1], z_eps like mu)")
        for (name, t), shape in zip(zip(("draws[0] (gamma)", "draws[1] (rho_eps)", "draws[2] (z_eps)"), draws), ((n, 2), (n, 1), (n, c, h, w))):
            if not isinstance(t, Tensor):
                raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
            if t.dtype != torch.float32:
                raise TypeError(f"{name} must be float32, got {t.dtype}")
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)}, got {tuple(t.shape)}")
            named.append((name, t))
    _check_devices(named)


def _upstream(g, shape, device) -> Tensor:
    """An upstream gradient as a contiguous fp32 tensor on the device (zeros for an output nothing depends on)."""
    if g is None:
        return torch.zeros(tuple(shape), dtype=torch.float32, device=device)
    g = g.detach()
    if g.dtype != torch.float32:
        g = g.float()
    return g.contiguous()


def _refuse_double_backward() -> None:
    if torch.is_grad_enabled():
        raise RuntimeError("elbo.elbo_sisr: double backward (create_graph=True) is not supported -- the backward runs on a HIP "
                           "kernel outside autograd and is first-order only")


class _SisrHead(torch.autograd.Function):
    """kinfo_est -> (kernel [N,1,k,k], kl_knet, kl_k0, kl_k1, kl_k2); differentiable: kernel and kl_knet, in kinfo_est."""
    @staticmethod
    def forward(ctx, kinfo_est: Tensor, kinfo_gt: Tensor, gamma: Tensor, rho_eps: Tensor, ksc: Tensor, r2: float, p0: float, p1: float, k: int,
                sf: int, shift: bool):
        est, gt, gam, eps = (t.detach().contiguous() for t in (kinfo_est, kinfo_gt, gamma, rho_eps))
        n = est.shape[0]
        lib = _native.load()
        with torch.cuda.device(est.device):
            ws = torch.empty(lib.virnet_sisr_head_workspace_bytes(n) // 8, dtype=torch.float64, device=est.device)
            kernel = torch.empty((n, 1, k, k), dtype=torch.float32, device=est.device)
            out = torch.empty(4, dtype=torch.float32, device=est.device)
            _native.check(lib.virnet_sisr_head_forward(est.data_ptr(), gt.data_ptr(), gam.data_ptr(), eps.data_ptr(), ksc.data_ptr(), r2, p0, p1, k, sf,
                                                       int(shift), ws.data_ptr(), kernel.data_ptr(), out.data_ptr(), n, _native.stream_handle()),
                          "sisr_head_forward")
        ctx.consts = (r2, p0, p1, k, sf, int(shift))
        ctx.save_for_backward(est, gt, gam, eps, ksc)
        knet, k0, k1, k2 = out.unbind(0)
        ctx.mark_non_differentiable(k0, k1, k2)
        return kernel, knet, k0, k1, k2

    @staticmethod
    def backward(ctx, g_kernel, g_knet, *_unused):
        _refuse_double_backward()
        est, gt, gam, eps, ksc = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 11
        r2, p0, p1, k, sf, shift = ctx.consts
        n = est.shape[0]
        with torch.cuda.device(est.device):
            gk = _upstream(g_kernel, (n, 1, k, k), est.device)
            gs = _upstream(g_knet, (), est.device)
            dkinfo = torch.empty((n, 3), dtype=torch.float32, device=est.device)
            _native.check(_native.load().virnet_sisr_head_backward(est.data_ptr(), gt.data_ptr(), gam.data_ptr(), eps.data_ptr(), ksc.data_ptr(),
                                                                   gk.data_ptr(), gs.data_ptr(), r2, p0, p1, k, sf, shift, dkinfo.data_ptr(), n,
                                                                   _native.stream_handle()), "sisr_head_backward")
        return (dkinfo,) + (None,) * 10


class _SisrHR(torch.autograd.Function):
    """mu -> (zz = mu + sqrt(eps2) z_eps, kl_rnet); differentiable in mu."""
    @staticmethod
    def forward(ctx, mu: Tensor, im_hr: Tensor, z_eps: Tensor, eps2: float):
        m, t, z = (x.detach().contiguous() for x in (mu, im_hr, z_eps))
        n, c, h, w = m.shape
        lib = _native.load()
        with torch.cuda.device(m.device):
            ws = torch.empty(lib.virnet_sisr_hr_workspace_bytes(n, c, h, w) // 8, dtype=torch.float64, device=m.device)
            zz = torch.empty((n, c, h, w), dtype=torch.float32, device=m.device)
            out = torch.empty(1, dtype=torch.float32, device=m.device)
            _native.check(lib.virnet_sisr_hr_value(m.data_ptr(), t.data_ptr(), z.data_ptr(), eps2, ws.data_ptr(), zz.data_ptr(), out.data_ptr(), n, c, h, w,
                                                   _native.stream_handle()), "sisr_hr_value")
        ctx.eps2 = eps2
        ctx.save_for_backward(m, t)
        return zz, out[0]

    @staticmethod
    def backward(ctx, g_zz, g_rnet):
        _refuse_double_backward()
        m, t = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        n, c, h, w = m.shape
        with torch.cuda.device(m.device):
            gz = _upstream(g_zz, m.shape, m.device)
            gs = _upstream(g_rnet, (), m.device)
            dmu = torch.empty((n, c, h, w), dtype=torch.float32, device=m.device)
            _native.check(_native.load().virnet_sisr_hr_grad(m.data_ptr(), t.data_ptr(), gz.data_ptr(), gs.data_ptr(), ctx.eps2, dmu.data_ptr(), n, c, h, w,
                                                             _native.stream_handle()), "sisr_hr_grad")
        return dmu, None, None, None


def _lr_layout(t: Tensor, h: int, w: int) -> Tuple[int, int]:
    """(channels, has the h x w plane) of a sigma tensor: [N,1,1,1] is one value per sample unless the image itself is 1 x 1"""
    full = tuple(t.shape[2:]) == (h, w)
    return int(t.shape[1]), int(full)


class _SisrLR(torch.autograd.Function):
    """(y, sigma_est) -> (lh, kl_snet); differentiable in both."""
    @staticmethod
    def forward(ctx, y: Tensor, sigma_est: Tensor, im_lr: Tensor, sigma_prior: Tensor, sc: Tensor):
        yy, sig, x, pri = (t.detach().contiguous() for t in (y, sigma_est, im_lr, sigma_prior))
        n, c, h, w = x.shape
        (cs, fs), (cp, fp) = _lr_layout(sig, h, w), _lr_layout(pri, h, w)
        lib = _native.load()
        with torch.cuda.device(x.device):
            ws = torch.empty(lib.virnet_sisr_lr_workspace_bytes(n, c, h, w) // 8, dtype=torch.float64, device=x.device)
            stats = torch.empty((n, 2), dtype=torch.float64, device=x.device)
            out = torch.empty(2, dtype=torch.float32, device=x.device)
            _native.check(lib.virnet_sisr_lr_value(yy.data_ptr(), x.data_ptr(), sig.data_ptr(), pri.data_ptr(), sc.data_ptr(), sc.data_ptr() + 4,
                                                   ws.data_ptr(), stats.data_ptr(), out.data_ptr(), n, c, h, w, cs, fs, cp, fp, _native.stream_handle()),
                          "sisr_lr_value")
        ctx.layout = (cs, fs, cp, fp)
        ctx.save_for_backward(yy, sig, x, pri, sc, stats)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_lh, g_snet):
        _refuse_double_backward()
        yy, sig, x, pri, sc, stats = ctx.saved_tensors
        need_y, need_sig = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_y or need_sig):
            return None, None, None, None, None
        n, c, h, w = x.shape
        cs, fs, cp, fp = ctx.layout
        with torch.cuda.device(x.device):
            gl, gs = _upstream(g_lh, (), x.device), _upstream(g_snet, (), x.device)
            dy = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
            dsig = torch.empty(tuple(sig.shape), dtype=torch.float32, device=x.device)
            _native.check(_native.load().virnet_sisr_lr_grad(yy.data_ptr(), x.data_ptr(), sig.data_ptr(), pri.data_ptr(), sc.data_ptr(), stats.data_ptr(),
                                                             gl.data_ptr(), gs.data_ptr(), dy.data_ptr(), dsig.data_ptr(), n, c, h, w, cs, fs, cp, fp,
                                                             _native.stream_handle()), "sisr_lr_grad")
        return (dy if need_y else None), (dsig if need_sig else None), None, None, None


class _SisrSum(torch.autograd.Function):
    """loss = lh + kl_rnet + kl_snet + kl_knet in fp32, in that order: one launch; the upstream gradient passes to the four terms unchanged."""
    @staticmethod
    def forward(ctx, lh: Tensor, rnet: Tensor, snet: Tensor, knet: Tensor):
        with torch.cuda.device(lh.device):
            out = torch.empty(1, dtype=torch.float32, device=lh.device)
            _native.check(_native.load().virnet_sisr_finish(lh.data_ptr(), rnet.data_ptr(), snet.data_ptr(), knet.data_ptr(), out.data_ptr(),
                                                            _native.stream_handle()), "sisr_finish")
        return out[0]

    @staticmethod
    def backward(ctx, g):
        _refuse_double_backward()
        return g, g, g, g


def elbo_sisr(mu: Tensor, sigma_est: Tensor, kinfo_est: Tensor, im_hr: Tensor, im_lr: Tensor, sigma_prior: Tensor, alpha0, kinfo_gt: Tensor,
              kappa0, r2: float, eps2: float, sf: int, k_size: int, penalty_K: Sequence[float], shift: bool, downsampler: str,
              degrade_impl: str = "hip", draws=None) -> Tuple[Tensor, List[Tensor]]:
    """``(loss, [lh, kl_rnet, kl_snet, kl_knet, kl_k0, kl_k1, kl_k2, kernel])`` of ``loss.elbo_sisr`` (loss/ELBO_simple.py:82-138, called as
    in train_SISR.py:207-224): 0-dim fp32 CUDA tensors and the detached [N,1,k,k] kernel.

    ``mu``, ``im_hr`` [N,C,H,W]; ``im_lr`` [N,C,ceil(H/sf),ceil(W/sf)]; ``sigma_est`` and ``sigma_prior`` each [N,1,1,1], [N,1,h,w] or
    [N,C,h,w] at the LR size, broadcast as the torch expressions broadcast them; ``kinfo_est``, ``kinfo_gt`` [N,3].  ``alpha0`` and
    ``kappa0``: a one-element fp32 tensor on the device or a Python float.  ``k_size`` at most 25 with k_size // 2 < min(H, W), ``sf`` 1..4.
    ``degrade_impl``: "hip" (``degrade.blur_downsample``, reflect border, odd ``k_size``) or "torch" (``loss.blur_downsample``); the
    degradation is its own autograd node between the HR and the LR pass.

    ``draws=None`` takes the three draws from torch's generator on the tensors' device in the reference's order and with its primitives
    (the standard-Gamma draw of ``Gamma(kappa0 - 1, .).rsample()`` floored at the dtype's tiny, ``randn`` [N,1], ``randn_like(mu)``): the
    same seed gives the draws ``loss.elbo_sisr`` makes on that device.  ``draws=(gamma [N,2], rho_eps [N,1], z_eps like mu)`` supplies them
    (CUDA fp32) and leaves the generator alone.

    ``loss`` is differentiable (first order) in ``mu``, ``sigma_est`` and ``kinfo_est``; the listed parts carry no gradient.

    One documented difference from the torch route: a sample whose 2x2 covariance has a determinant of exactly zero (or a non-finite one) in
    fp64 gets 1e-5 added to both diagonal entries -- that sample only.  The torch route nudges the whole batch, and only when LAPACK
    reports a zero pivot.  Per sample keeps a sample's bits independent of its batch neighbours.

    Argument errors are raised before any device work.  The first call for a shape may upload constants (bicubic tap tables, Python-float
    ``alpha0`` / ``kappa0``); after that nothing synchronises: warm a shape up before capturing it into a graph."""
    _check_sisr_args(mu, sigma_est, kinfo_est, im_hr, im_lr, sigma_prior, alpha0, kinfo_gt, kappa0, r2, eps2, sf, k_size, penalty_K, downsampler,
                     degrade_impl, draws)
    dev = mu.device
    with torch.no_grad(), torch.cuda.device(dev):
        sc = _scalars(alpha0, dev)
        ksc = kappa0.detach().reshape(1) if isinstance(kappa0, Tensor) else _device_float(float(kappa0), str(dev))
        if draws is None:
            conc = torch.ones_like(kinfo_est[:, :2]) * (ksc - 1)
            gamma = torch._standard_gamma(conc).clamp_(min=torch.finfo(torch.float32).tiny)      # what Gamma.rsample draws, before / rate
            rho_eps = torch.randn_like(kinfo_est[:, 2].unsqueeze(1))
            z_eps = torch.randn_like(mu)
        else:
            gamma, rho_eps, z_eps = draws
    kernel, knet, k0, k1, k2 = _SisrHead.apply(kinfo_est, kinfo_gt, gamma, rho_eps, ksc, float(r2), float(penalty_K[0]), float(penalty_K[1]),
                                               int(k_size), int(sf), bool(shift))
    zz, rnet = _SisrHR.apply(mu, im_hr, z_eps, float(eps2))
    if degrade_impl == "hip":
        from . import degrade
        y = degrade.blur_downsample(zz, kernel, sf, downsampler, border="reflect")
    else:
        from . import loss as _loss
        y = _loss.blur_downsample(zz, kernel, sf, downsampler, impl="torch")
    lh, snet = _SisrLR.apply(y, sigma_est, im_lr, sigma_prior, sc)
    total = _SisrSum.apply(lh, rnet, snet, knet)
    return total, [lh.detach(), rnet.detach(), snet.detach(), knet.detach(), k0, k1, k2, kernel.detach()]
