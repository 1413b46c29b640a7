"""The real-noise benchmarks (SIDD blocks, DND boxes) around the device-side self-ensemble (virnet_amd/ensemble.py).

Restated, not copied, from scripts/denoising_virnet_real_sidd.py:97-164 and scripts/denoising_virnet_real_dnd.py +
dnd_submission_py/pytorch_wrapper.py:15-47:

  * SIDD: every 256 x 256 uint8 block of the ``[I,K,H,W,3]`` ``.mat`` array is restored, with ``--flip`` (the default) as the mean of
    the eight back-transformed restorations of its eight orientations in the script's sequential float32 order, then
    ``img_as_ubyte(clip(.))``; with the ground-truth blocks, PSNR and SSIM on uint8 RGB with border 0 per block and their means.
  * DND: a float32 ``[H,W,3]`` crop is restored the same way with the wrapper's ``mean(axis=3)`` (pairwise order), clipped, not quantised.

``sidd_blocks`` / ``dnd_box`` run on the device: the orientations of ``batch // 8`` blocks are one forward batch, the metrics are
``metrics.psnr_ssim``, and the host waits once, at the end.  ``sidd_blocks_np`` / ``dnd_box_np`` are the same tables through
``ensemble.restore_np`` and the host metrics, for any ``forward`` on numpy arrays.  Not reproduced: the scripts' timing, their ``thop`` FLOP
count and LPIPS.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from . import ensemble, metrics
from . import eval as veval


def _blocks(noisy: np.ndarray, gt: Optional[np.ndarray]):
    noisy = np.ascontiguousarray(noisy)          # (scipy.io.loadmat hands out Fortran-ordered arrays)
    if noisy.ndim != 5 or noisy.dtype != np.uint8 or noisy.shape[-1] != 3:
        raise ValueError(f"noisy must be uint8 [I,K,H,W,3] (the .mat array), got {noisy.dtype} {noisy.shape}")
    if gt is not None:
        gt = np.ascontiguousarray(gt)
        if gt.shape != noisy.shape or gt.dtype != np.uint8:
            raise ValueError(f"gt must be uint8 {noisy.shape} like noisy, got {gt.dtype} {gt.shape}")
    return noisy, gt


def _table(res: dict, shape, psnrs, ssims) -> dict:
    """The script's running sums (:110,153-159): per-block values in block order, means as sum / count."""
    res["psnr"] = np.asarray(psnrs, dtype=np.float64).reshape(shape)
    res["ssim"] = np.asarray(ssims, dtype=np.float64).reshape(shape)
    res["psnr_mean"] = float(sum(psnrs) / len(psnrs))
    res["ssim_mean"] = float(sum(ssims) / len(ssims))
    return res


def _net_forward(net) -> Callable:
    def forward(x):
        with torch.no_grad():
            return net(x)[0]
    return forward


def sidd_blocks(net, noisy: np.ndarray, gt: Optional[np.ndarray] = None, flip: bool = True, batch: int = 8) -> dict:
    """Restore every block of the SIDD array ``noisy`` (uint8 ``[I,K,H,W,3]``) with ``net`` (``net(x)[0]`` is the restoration) on the
    device.  Returns ``{"denoised": uint8 like noisy}`` (the script's ``denoised_res``) and, with the ground truth ``gt``, ``"psnr"`` /
    ``"ssim"`` (float64 ``[I,K]``) and ``"psnr_mean"`` / ``"ssim_mean"``.  ``batch``: the most images one forward sees, i.e. ``batch // 8``
    blocks at a time with ``flip`` (at least one).  Both arrays go to the device once; the host waits once, for the results."""
    noisy, gt = _blocks(noisy, gt)
    ni, nk, h, w, c = noisy.shape
    n = ni * nk
    per = max(1, int(batch) // (8 if flip else 1))
    forward = _net_forward(net)
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if dev is None:
        raise RuntimeError("no ROCm device: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    src = torch.from_numpy(np.ascontiguousarray(noisy.reshape(n, h, w, c))).to(dev)
    ref = None if gt is None else torch.from_numpy(np.ascontiguousarray(gt.reshape(n, h, w, c).transpose(0, 3, 1, 2))).to(dev)
    stored, pending = [], []
    for a in range(0, n, per):
        b = min(a + per, n)
        groups = ensemble.restored_groups(forward, ensemble.expand(src[a:b], flip), batch)
        stored.append(ensemble.reduce(*groups, order="sequential", out="uint8", layout="hwc"))
        if ref is not None:
            pending.append(metrics.psnr_ssim(ensemble.reduce(*groups, order="sequential", out="uint8", layout="chw"), ref[a:b]))
    res = {"denoised": torch.cat(stored).cpu().numpy().reshape(noisy.shape)}
    if ref is None:
        return res
    psnrs, ssims = metrics.table_collect(pending, True)
    return _table(res, (ni, nk), psnrs, ssims)


def sidd_blocks_np(forward: Callable[[np.ndarray], np.ndarray], noisy: np.ndarray, gt: Optional[np.ndarray] = None, flip: bool = True,
                   batch: int = 8) -> dict:
    """:func:`sidd_blocks` on the host for any ``forward: float32 [n,3,h,w] -> float32 [n,3,h,w]``: ``ensemble.restore_np`` per block,
    ``eval.calculate_psnr`` / ``calculate_ssim``."""
    noisy, gt = _blocks(noisy, gt)
    ni, nk = noisy.shape[:2]
    den = np.zeros_like(noisy)
    psnrs, ssims = [], []
    for i in range(ni):
        for k in range(nk):
            den[i, k] = ensemble.restore_np(forward, noisy[i, k][np.newaxis], flip, "sequential", "uint8", "hwc", batch)[0]
            if gt is not None:
                psnrs.append(veval.calculate_psnr(gt[i, k], den[i, k], border=0))
                ssims.append(veval.calculate_ssim(gt[i, k], den[i, k], border=0))
    res = {"denoised": den}
    return res if gt is None else _table(res, (ni, nk), psnrs, ssims)


def _crop(crop: np.ndarray) -> np.ndarray:
    crop = np.asarray(crop)
    if crop.ndim != 3 or crop.dtype != np.float32 or crop.shape[-1] != 3:
        raise ValueError(f"crop must be float32 [H,W,3], got {crop.dtype} {crop.shape}")
    return crop


def dnd_box(net, crop: np.ndarray, flip: bool = True) -> np.ndarray:
    """One DND bounding box: float32 ``[H,W,3]`` in, the clipped float32 restoration out -- what ``pytorch_denoiser(...)`` returns, so
    ``lambda crop, nlf: dnd_box(net, crop)`` is the ``denoiser`` that ``denoise_srgb`` takes."""
    crop = _crop(crop)
    return ensemble.restore(_net_forward(net), crop[np.newaxis], flip, "pairwise", "float32", "hwc")[0].cpu().numpy()


def dnd_box_np(forward: Callable[[np.ndarray], np.ndarray], crop: np.ndarray, flip: bool = True) -> np.ndarray:
    """:func:`dnd_box` on the host."""
    return ensemble.restore_np(forward, _crop(crop)[np.newaxis], flip, "pairwise", "float32", "hwc")[0]
