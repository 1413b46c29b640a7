"""SISR evaluation harness around the hot path (SURVEY.md 8-a11 iii / 8-f2): the synthetic degradation the reference's
``scripts/sisr_virnet_syn.py:99-137`` applies to a ground-truth image before calling ``net(lr, sf)``.

Own restatements (numpy / scipy only), pinned by tests/golden/sisr_harness.npz which the reference's helpers produced:

  * ``anisotropic_gaussian_kernel``  -- utils/util_sisr.py:60-92 (softmax of the quadratic form on a k x k grid)
  * ``test_kernels``                 -- the seven kernels of scripts/sisr_virnet_syn.py:103-116
  * ``bicubic_downscale``            -- the antialiased cubic resampler the reference vendors as ResizeRight/
                                        (Shocher et al., "From Discrete to Continuous Convolution Layers"): output sample i sits at
                                        i/s + (n_in-1)/2 - (n_out-1)/(2 s), the cubic is stretched by 1/s, taps are mirrored at the
                                        borders (weights evaluated at the mirrored positions) and normalised
                                        to sum 1  (ResizeRight/resize_right.py:262-318)
  * ``degrade``                      -- utils/util_sisr.py:146-177: blur (true convolution, half-sample symmetric border), clip,
                                        downsample, seeded Gaussian noise in float64, cast to fp32, clip, and with ``qf`` the JPEG
                                        round trip of eval.jpeg_compress
  * ``synthesize_lr_np``             -- the tail of datasets/SISRDatasets.py:89-112 for one training sample whose kernel and noise the
                                        caller drew: blur, clip, downsample, fp32 noise, clip, JPEG round trip
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np
from scipy import ndimage

KERNEL_SIZE = 21          # scripts/sisr_virnet_syn.py:92
NOISE_SEED = 1234         # utils/util_sisr.py:146


def modcrop(im: np.ndarray, sf: int) -> np.ndarray:
    h, w = im.shape[:2]
    return im[:h - h % sf, :w - w % sf]


def anisotropic_gaussian_kernel(k_size: int, sf: int, lambda_1: float, lambda_2: float, theta: float,
                                shift: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(kernel [k,k] float64 summing to 1, (var_x, var_y, rho))."""
    c, s = math.cos(theta), math.sin(theta)
    rot = np.array([[c, -s], [s, c]])
    cov = rot @ np.diag([lambda_1, lambda_2]) @ rot.T
    prec = np.linalg.inv(cov)
    center = k_size // 2 + (0.5 * (sf - k_size % 2) if shift else 0.0)
    # the grid is built in fp32 (util_sisr.py:79) and only then promoted, so a half-pixel centre stays exact
    g = (np.arange(k_size, dtype=np.float32) - np.float32(center)).astype(np.float64)
    dx, dy = np.meshgrid(g, g)                                        # dx varies along columns
    q = -0.5 * (prec[0, 0] * dx * dx + (prec[0, 1] + prec[1, 0]) * dx * dy + prec[1, 1] * dy * dy)
    q -= q.max()
    e = np.exp(q)
    kernel = e / e.sum()
    rho = cov[0, 1] / (math.sqrt(cov[0, 0]) * math.sqrt(cov[1, 1]))
    return kernel, np.array([cov[0, 0], cov[1, 1], rho])


def test_kernels(sf: int, k_size: int = KERNEL_SIZE) -> List[np.ndarray]:
    spec = [(0.40, 0.40, 0.0), (0.60, 0.60, 0.0), (0.80, 0.80, 0.0), (0.4, 0.2, 0.0),
            (0.6, 0.3, 0.75 * np.pi), (0.8, 0.4, 0.25 * np.pi), (0.8, 0.4, 0.50 * np.pi)]
    return [anisotropic_gaussian_kernel(k_size, sf, (a * sf) ** 2, (b * sf) ** 2, th, False)[0] for a, b, th in spec]


test_kernels.__test__ = False      # not a pytest case


def _cubic(x: np.ndarray) -> np.ndarray:
    a = np.abs(x)
    a2, a3 = a * a, a * a * a
    return (1.5 * a3 - 2.5 * a2 + 1.0) * (a <= 1.0) + (-0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0) * ((a > 1.0) & (a <= 2.0))


def resample_taps(n_in: int, scale: float, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """The tap table of the antialiased cubic along one axis: ``out[o] = sum_t wgt[o, t] * in[idx[o, t]]`` with ``idx`` int64 and ``wgt``
    float64, both [n_out, taps] (ResizeRight/resize_right.py:262-318).  The one construction behind :func:`bicubic_downscale`,
    ``loss._bicubic_matrix`` and the device tables of ``virnet_amd.degrade``."""
    eps = float(np.finfo(np.float32).eps)
    support = 4.0 / scale if scale < 1.0 else 4.0                     # antialiasing widens the cubic when shrinking
    pos = np.arange(n_out) / scale + (n_in - 1) / 2 - (n_out - 1) / (2 * scale)
    left = np.ceil(pos - support / 2 - eps).astype(np.int64)
    taps = left[:, None] + np.arange(math.ceil(support - eps))
    mirror = np.concatenate([np.arange(n_in), np.arange(n_in - 1, -1, -1)])
    idx = mirror[np.remainder(taps, 2 * n_in)]
    d = pos[:, None] - idx                 # distances to the MIRRORED sample positions, as the reference computes them (:307)
    wgt = scale * _cubic(scale * d) if scale < 1.0 else _cubic(d)
    tot = wgt.sum(1, keepdims=True)
    tot[tot == 0] = 1
    return idx, wgt / tot


def _resample_axis0(x: np.ndarray, scale: float, n_out: int) -> np.ndarray:
    idx, wgt = resample_taps(x.shape[0], scale, n_out)
    return (x[idx] * wgt.reshape(wgt.shape + (1,) * (x.ndim - 1))).sum(1)


def bicubic_downscale(im: np.ndarray, sf: int) -> np.ndarray:
    """[h,w,c] -> [ceil(h/sf), ceil(w/sf), c], float64 (fp32 samples times float64 taps)."""
    scale = 1.0 / sf
    out = _resample_axis0(im, scale, math.ceil(scale * im.shape[0]))
    out = np.swapaxes(_resample_axis0(np.swapaxes(out, 0, 1), scale, math.ceil(scale * im.shape[1])), 0, 1)
    return out


def degrade(im_hr: np.ndarray, kernel: np.ndarray, sf: int, nlevel: float = 2.55, seed: int = NOISE_SEED,
            downsampler: str = "bicubic", qf=None) -> np.ndarray:
    """fp32 [h,w,3] in [0,1] -> LR fp32 [h/sf, w/sf, 3].  ``qf``: JPEG quality of a final round trip (util_sisr.py:173-175), None for none."""
    if im_hr.dtype != np.float32:
        raise TypeError("degrade expects a float32 image in [0,1]")
    blur = ndimage.convolve(im_hr, kernel[:, :, None], mode="reflect")
    blur = np.clip(blur, 0.0, 1.0)
    mode = downsampler.lower()
    if mode == "direct":
        lr = blur[::sf, ::sf].astype(np.float64)                      # noise is float64, so the sum below is too
    elif mode == "bicubic":
        lr = bicubic_downscale(blur, sf)
    else:
        raise ValueError("downsampler must be 'direct' or 'bicubic'")
    lr = lr + np.random.default_rng(seed).standard_normal(size=lr.shape) * (nlevel / 255.0)
    lr = np.clip(lr.astype(np.float32), 0.0, 1.0)
    if qf is not None:
        from . import eval as veval
        lr = veval.jpeg_compress(lr, int(qf))
    return lr


def synthesize_lr_np(im_hr: np.ndarray, kernel: np.ndarray, sf: int, noise: np.ndarray, std: float, qf: int = 0,
                     downsampler: str = "bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """The tail of GeneralTrainFloder.__getitem__ (datasets/SISRDatasets.py:89-112) for one sample: fp32 [h,w,3] ``im_hr`` in [0,1], the
    [k,k] ``kernel`` as the dataset makes it (applied as a true convolution), standard-normal fp32 ``noise`` [h/sf,w/sf,3], its level
    ``std`` and the JPEG quality ``qf`` (0: none) -> (im_lr, im_blur), both fp32 [h/sf,w/sf,3].  im_blur is the clipped blur downsampled;
    im_lr = clip(im_blur + noise * std, 0, 1) in fp32, then the round trip.  The host counterpart of ``degrade.synthesize_lr``."""
    if im_hr.dtype != np.float32:
        raise TypeError("synthesize_lr_np expects a float32 image in [0,1]")
    blur = np.clip(ndimage.convolve(im_hr, np.asarray(kernel)[:, :, None], mode="reflect"), 0.0, 1.0)
    mode = downsampler.lower()
    if mode == "direct":
        im_blur = np.ascontiguousarray(blur[::sf, ::sf])
    elif mode == "bicubic":
        im_blur = bicubic_downscale(blur, sf).astype(np.float32)
    else:
        raise ValueError("downsampler must be 'direct' or 'bicubic'")
    return synthesize_tail_np(im_blur, noise, std, qf), im_blur


def synthesize_tail_np(im_blur: np.ndarray, noise: np.ndarray, std: float, qf: int = 0) -> np.ndarray:
    """``clip(im_blur + noise * std, 0, 1)`` in fp32, product and sum rounded separately, then the JPEG round trip when ``qf`` is not 0."""
    from . import eval as veval
    im_lr = np.clip(im_blur.astype(np.float32) + np.asarray(noise, dtype=np.float32) * np.float32(std), np.float32(0.0), np.float32(1.0))
    return veval.jpeg_compress(im_lr, int(qf)) if int(qf) else im_lr


def sisr_table(forward, data, sf: int, nlevel: float = 2.55, kernels=None, with_ssim: bool = True, device_metrics: bool = False,
               device_degrade: bool = False, qf=None, lpips=None):
    """The PSNR-Y / SSIM-Y table of scripts/sisr_virnet_syn.py:99-170 for any ``forward(lr float32 HWC, sf) -> sr float32 HWC``:
    per dataset and per test kernel (seven, :103-116), every ground-truth image is mod-cropped, blurred, bicubically downscaled,
    noised with the seeded stream (util_sisr.py:146-177) and restored; metrics on the uint8 Y channel with border sf**2 (:150).
    ``data`` = ["folder:ext", ...].  Returns rows {"dataset", "kernel", "psnr_y", "ssim_y", "images", "per_image_psnr_y"}.

    ``lpips``: a ``virnet_amd.lpips.LpipsWeights`` (``load_weights`` of the `lpips` package's exported AlexNet weights) adds the table's third
    column (:158-161,169): each row gains ``"lpips"`` (the mean) and ``"per_image_lpips"`` after the keys above, computed on the whole
    mod-cropped RGB image, no border crop -- on the host by ``lpips.distance_torch`` in float32, with ``device_metrics`` by
    ``lpips.table_pair`` on the same ``mu`` and within the same single synchronisation.  None (the default): the rows above, unchanged.

    ``device_metrics=True``: ``forward`` returns the un-clipped ``mu`` as a CUDA tensor [1,3,H,W] (or [3,H,W]) instead; clip, quantisation,
    luma, crop, PSNR-Y and SSIM-Y then run on the device (virnet_amd/metrics.py) with one synchronisation per (dataset, kernel).

    ``device_degrade=True``: blur, clip and bicubic downscale run on the device (virnet_amd/degrade.py; the seeded noise is still the host's
    stream) and ``forward`` receives the LR image as a CUDA tensor [1,3,h,w] instead of an HWC array.  Together with ``device_metrics`` an
    image does not leave the device between the ground truth's upload and its metrics.

    ``qf``: JPEG quality of a round trip that ends the degradation (the reference's GeneralTest evaluates at 40), on the host or, with
    ``device_degrade``, on the device (virnet_amd/jpeg.py); None (the default) for none."""
    import glob
    import os
    from . import eval as veval
    if device_metrics:
        from . import metrics
    if device_degrade:
        from . import degrade as device
    if lpips is not None:
        import torch
        from . import lpips as vlpips
        if not isinstance(lpips, vlpips.LpipsWeights):
            raise TypeError(f"lpips must be a virnet_amd.lpips.LpipsWeights or None, got {type(lpips).__name__}")
    kernels = test_kernels(sf) if kernels is None else kernels
    rows = []
    for spec in data:
        folder, ext = spec.rsplit(":", 1)
        files = sorted(glob.glob(os.path.join(folder, "*." + ext.lstrip("."))))
        if not files:
            continue
        for kidx, kernel in enumerate(kernels):
            psnrs, ssims, pending = [], [], []
            dists, dist_pending = [], []
            for f in files:
                gt = modcrop(veval.imread_rgb_uint8(f), sf)
                if device_degrade:
                    lr = device.degrade_lr(veval.img_as_float32(gt), kernel, sf, nlevel=nlevel, downsampler="bicubic", qf=qf)
                else:
                    lr = degrade(veval.img_as_float32(gt), kernel, sf, nlevel=nlevel, downsampler="bicubic", qf=qf)
                if device_metrics:
                    mu = forward(lr, sf)
                    pending.append(metrics.table_pair(mu, gt, sf ** 2, True, with_ssim))
                    if lpips is not None:
                        dist_pending.append(vlpips.table_pair(mu, gt, lpips))
                    continue
                sr = veval.img_as_ubyte(np.clip(forward(lr, sf), 0.0, 1.0))
                if lpips is not None:
                    pair = [torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[np.newaxis])) for im in (sr, gt)]
                    dists.append(float(vlpips.distance_torch(pair[0], pair[1], lpips, torch.float32)[0]))
                psnrs.append(veval.calculate_psnr_y(sr, gt, border=sf ** 2))
                if with_ssim:
                    ssims.append(veval.calculate_ssim(sr, gt, border=sf ** 2, ycbcr=True))
            if device_metrics:
                if lpips is not None:
                    dists = vlpips.table_collect(dist_pending)       # the queue is in order: this copy is the one synchronisation
                psnrs, ssims = metrics.table_collect(pending, with_ssim)
            rows.append({"dataset": os.path.basename(folder.rstrip("/")), "kernel": kidx + 1, "psnr_y": float(np.mean(psnrs)),
                         "ssim_y": float(np.mean(ssims)) if ssims else float("nan"), "images": len(files), "per_image_psnr_y": psnrs})
            if lpips is not None:
                rows[-1]["lpips"] = float(np.mean(dists))
                rows[-1]["per_image_lpips"] = dists
    return rows
