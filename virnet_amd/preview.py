"""Training previews on the device (csrc/preview.hip): the images and scalars the training scripts hand to their summary writer.

    g = grid(mu, clamp=(0.0, 1.0), channels=3)          # uint8 CUDA tensor [Hg, Wg, 3]: make_grid(normalize=True, scale_each=True) as the
                                                        # writer stores it; two launches, mu is not modified
    k = kernel_from_kinfo(kinfo, k_size=21, sf=4)       # util_sisr.kinfo2sigma: [N, 3] -> [N, 1, k, k]
    tags, grids = denoise_train(keep)                   # the five grids of train_denoising_syn.py:201-211 from a step's tensors
    for tag, im in zip(tags, to_host(grids)):           # ONE pinned copy and ONE event wait for the whole event
        writer.add_image(tag, im, step, dataformats="HWC")

:func:`grid_np` and :func:`kernel_np` are the definitions, in numpy; the kernels match the first bit for bit and the second to the last
bit of the device's fp64 ``exp``.  Two facts about ``grid_np``.  First: torchvision and tensorboard are not installed where this package
is built, so the definition is restated from their documented behaviour -- ``make_grid`` clones the batch, shifts and scales every image
by its own minimum and ``max(max - min, 1e-5)``, repeats a single plane three times, returns a single image as it is and otherwise lays
the images into a zero canvas ``padding`` pixels apart; the writer's conversion is ``(x * 255).clip(0, 255).astype(uint8)``, a truncation
-- and it cannot be pinned to either library there.  Second: torch's CUDA ``div_`` by a Python scalar multiplies by the scalar's
reciprocal, while the definition divides (one rounding), so the reference's own bits on a GPU can differ from the definition by one grey
level where a value sits at a truncation boundary.  The one specified departure is non-finite input, which the reference does not define
(its minimum would be NaN): NaN and -inf give 0, +inf gives 255, they are left out of the minimum and maximum, and an image without a
finite element is all zeros.  The deferred range guard poisons outputs with NaN, so the case is reachable.

The builders (:func:`denoise_train`, :func:`denoise_test`, :func:`sisr_train`, :func:`sisr_test`) are pure: they take tensors a training
step or a test forward already has and return the reference's tag strings and the grids, all of one event in ONE device buffer (a grid's
byte run may start at any address: the kernel stores aligned dwords with byte ends), so :func:`to_host` moves the event in one copy.

:class:`FolderWriter` is a summary writer that needs no tensorboard: PNG files and one JSON-lines file.  The loops of :mod:`fit` use a writer
through two calls only, ``add_scalar(tag, float, step)`` and ``add_image(tag, uint8 ndarray [H, W, 3], step, dataformats="HWC")``, which
``torch.utils.tensorboard.SummaryWriter`` and tensorboardX take unchanged.

CUDA float32 tensors only, no fallback.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _native

MAX_KERNEL = 25


# ---- the definitions -------------------------------------------------------------------------------------------------------------------------
def grid_shape(b: int, h: int, w: int, nrow: int = 8, padding: int = 2) -> Tuple[int, int, int, int]:
    """(Hg, Wg, xmaps, ymaps) of the grid of ``b`` images of ``h`` x ``w``; one image is its own grid, without a border."""
    if b < 1 or h < 1 or w < 1 or nrow < 1 or padding < 0:
        raise ValueError(f"grid: batch {b}, image {h}x{w}, nrow {nrow}, padding {padding}")
    if b == 1:
        return h, w, 1, 1
    xmaps = min(nrow, b)
    ymaps = -(-b // xmaps)
    return ymaps * (h + padding) + padding, xmaps * (w + padding) + padding, xmaps, ymaps


def grid_np(x, nrow: int = 8, padding: int = 2, clamp: Optional[Tuple[float, float]] = None) -> np.ndarray:
    """The definition of :func:`grid`: float32 [B, C, H, W], C 1 or 3 -> uint8 [Hg, Wg, 3] (module docstring)."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 4 or x.shape[1] not in (1, 3):
        raise TypeError(f"grid_np takes a float32 [B, 1 or 3, H, W] array, got {x.dtype} {x.shape}")
    b, c, h, w = x.shape
    hg, wg, xmaps, _ = grid_shape(b, h, w, nrow, padding)
    if clamp is not None:
        x = np.clip(x, np.float32(clamp[0]), np.float32(clamp[1]))                # NaN passes
    out = np.zeros((hg, wg, 3), dtype=np.uint8)
    for k in range(b):
        v = x[k]
        fin = np.isfinite(v)
        if not fin.any():
            continue
        lo, hi = v[fin].min(), v[fin].max()
        d = np.float32(max(float(hi) - float(lo), 1e-5))
        with np.errstate(all="ignore"):
            y = np.divide(np.subtract(v, lo, dtype=np.float32), d, dtype=np.float32)
            t = np.multiply(y, np.float32(255.0), dtype=np.float32)
            t = np.where(t > 0, np.minimum(t, np.float32(255.0)), np.float32(0.0))          # clip; NaN -> 0
        u = np.broadcast_to(t.astype(np.uint8), (3, h, w)) if c == 1 else t.astype(np.uint8)   # astype truncates
        y0, x0 = (0, 0) if b == 1 else ((k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding)
        out[y0:y0 + h, x0:x0 + w] = u.transpose(1, 2, 0)
    return out


def kernel_centre(k_size: int, sf: int, shift: bool) -> float:
    return k_size // 2 + (0.5 * (sf - k_size % 2) if shift else 0.0)


def kernel_f64_np(kinfo, k_size: int, sf: int, shift: bool = False) -> np.ndarray:
    """:func:`kernel_np` before its rounding to float32: float64 [N, 1, k, k]."""
    return _kernel_f64(kinfo, k_size, sf, shift)


def kernel_np(kinfo, k_size: int, sf: int, shift: bool = False) -> np.ndarray:
    """The definition of :func:`kernel_from_kinfo` (util_sisr.py:26-58, 95-107) in fp64, returned as float32 [N, 1, k, k]: the covariance
    [[v1, d], [d, v2]], d = sqrt(v1) sqrt(v2) rho, its closed-form inverse, and a softmax of -0.5 z' S^-1 z over the positions z = (row,
    column) - centre.  A sample whose determinant is exactly zero or not finite gets 1e-5 on both diagonal entries, that sample only
    (``elbo.elbo_sisr`` documents the rule; the reference nudges the whole batch when its inverse fails)."""
    return _kernel_f64(kinfo, k_size, sf, shift).astype(np.float32)


def _kernel_f64(kinfo, k_size: int, sf: int, shift: bool) -> np.ndarray:
    kinfo = np.asarray(kinfo, dtype=np.float64)
    if kinfo.ndim != 2 or kinfo.shape[1] != 3:
        raise TypeError(f"kernel_np takes [N, 3], got {kinfo.shape}")
    k = int(k_size)
    with np.errstate(all="ignore"):
        v1, v2, rho = kinfo[:, 0], kinfo[:, 1], kinfo[:, 2]
        d = np.sqrt(v1) * np.sqrt(v2) * rho
        det = v1 * v2 - d * d
        bad = (det == 0.0) | ~np.isfinite(det)
        s1, s2 = np.where(bad, v1 + 1e-5, v1), np.where(bad, v2 + 1e-5, v2)
        det = np.where(bad, s1 * s2 - d * d, det)
        a00, a01, a11 = s2 / det, -d / det, s1 / det
        z = np.arange(k, dtype=np.float64) - kernel_centre(k, sf, shift)
        zr, zc = z[None, :, None], z[None, None, :]
        q = -0.5 * (zr * zr * a00[:, None, None] + 2.0 * zr * zc * a01[:, None, None] + zc * zc * a11[:, None, None])
        e = np.exp(q - q.max(axis=(1, 2), keepdims=True))
        out = e / e.sum(axis=(1, 2), keepdims=True)
    return out[:, None]


# ---- the device functions --------------------------------------------------------------------------------------------------------------------
def _check_batch(x, channels: Optional[int], who: str) -> Tuple[int, int, int, int, int]:
    """(b, c, h, w, batch stride) of a batch the kernel reads in place: the first ``c`` planes of every image are one dense run."""
    if not isinstance(x, Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise TypeError(f"{who}: a CUDA float32 [B, C, H, W] tensor is expected, got "
                        f"{type(x).__name__ if not isinstance(x, Tensor) else (x.device, x.dtype, tuple(x.shape))}")
    b, cx, h, w = x.shape
    c = cx if channels is None else int(channels)
    if c not in (1, 3) or c > cx:
        raise ValueError(f"{who}: {c} channels of a batch with {cx} (1 or 3 expected)")
    if b < 1 or h < 1 or w < 1:
        raise ValueError(f"{who}: empty batch {tuple(x.shape)}")
    sb, sc, sh, sw = x.stride()
    if (w > 1 and sw != 1) or (h > 1 and sh != w) or (c > 1 and sc != h * w) or (b > 1 and sb < c * h * w):
        raise ValueError(f"{who}: strides {tuple(x.stride())} of shape {tuple(x.shape)}: every image's first {c} planes must be dense NCHW")
    return b, c, h, w, (sb if b > 1 else c * h * w)


def _grid_into(out: Tensor, x: Tensor, dims, nrow: int, padding: int, clamp) -> None:
    b, c, h, w, sb = dims
    lib = _native.load()
    lo, hi = (0.0, 0.0) if clamp is None else (float(np.float32(clamp[0])), float(np.float32(clamp[1])))
    with torch.cuda.device(x.device):
        ws = torch.empty(lib.virnet_preview_grid_workspace_bytes(b) // 4, dtype=torch.float32, device=x.device)
        _native.check(lib.virnet_preview_grid(_native.ptr(x), sb, b, c, h, w, nrow, padding, int(clamp is not None), lo, hi, _native.ptr(ws),
                                              _native.ptr(out), out.shape[0], out.shape[1], _native.stream_handle()), "preview.grid")


def grids(specs: Sequence[dict]) -> List[Tensor]:
    """The grids of one event, in ONE uint8 device buffer (so :func:`to_host` is one copy).  ``specs``: per grid the keywords of
    :func:`grid` as a dict with the batch under ``"x"``.  Two launches per grid, nothing synchronises."""
    if not specs:
        return []
    plans = []
    for s in specs:
        nrow, padding = int(s.get("nrow", 8)), int(s.get("padding", 2))
        dims = _check_batch(s["x"], s.get("channels"), "preview.grid")
        clamp = s.get("clamp")
        if clamp is not None and not float(clamp[0]) <= float(clamp[1]):
            raise ValueError(f"preview.grid: clamp {clamp!r}: an increasing pair is expected")
        hg, wg, _, _ = grid_shape(dims[0], dims[2], dims[3], nrow, padding)
        if hg * wg * 3 >= 1 << 31 or dims[0] * dims[4] >= 1 << 31:
            raise ValueError(f"preview.grid: the batch {tuple(s['x'].shape)} or its grid {hg}x{wg}x3 reaches 2^31 elements")
        if s["x"].device != specs[0]["x"].device:
            raise RuntimeError("preview.grids: the batches of one event must be on one device")
        plans.append((s["x"], dims, nrow, padding, clamp, hg, wg))
    with torch.no_grad(), torch.cuda.device(specs[0]["x"].device):
        buf = torch.empty(sum(p[5] * p[6] * 3 for p in plans), dtype=torch.uint8, device=specs[0]["x"].device)
        out, at = [], 0
        for x, dims, nrow, padding, clamp, hg, wg in plans:
            g = buf[at:at + hg * wg * 3].view(hg, wg, 3)
            _grid_into(g, x.detach(), dims, nrow, padding, clamp)
            out.append(g)
            at += hg * wg * 3
    return out


def grid(x: Tensor, nrow: int = 8, padding: int = 2, clamp: Optional[Tuple[float, float]] = None, channels: Optional[int] = None) -> Tensor:
    """``make_grid(x, nrow, padding, normalize=True, scale_each=True)`` as the summary writer stores it: a uint8 CUDA tensor [Hg, Wg, 3]
    (:func:`grid_np` is the definition).  ``clamp``: (lo, hi), applied to every element as it is loaded -- the reference's in-place
    ``clamp_`` without the write.  ``channels``: preview the first so many channels of a wider batch, in place."""
    return grids([dict(x=x, nrow=nrow, padding=padding, clamp=clamp, channels=channels)])[0]


def kernel_from_kinfo(kinfo: Tensor, k_size: int, sf: int, shift: bool = False) -> Tensor:
    """``util_sisr.kinfo2sigma(kinfo, k_size, sf, shift)``: CUDA float32 [N, 3] (variance x, variance y, rho) -> [N, 1, k, k], in fp64 on
    the device, one launch (:func:`kernel_np` is the definition)."""
    if not isinstance(kinfo, Tensor) or not kinfo.is_cuda or kinfo.dtype != torch.float32 or kinfo.dim() != 2 or kinfo.shape[1] != 3 or not len(kinfo):
        raise TypeError("preview.kernel_from_kinfo: a CUDA float32 [N, 3] tensor with N >= 1 is expected")
    k_size, sf = int(k_size), int(sf)
    if not 1 <= k_size <= MAX_KERNEL or sf < 1:
        raise ValueError(f"preview.kernel_from_kinfo: k_size {k_size} (1..{MAX_KERNEL} expected), sf {sf}")
    with torch.no_grad(), torch.cuda.device(kinfo.device):
        src = kinfo.detach().contiguous()
        out = torch.empty((len(src), 1, k_size, k_size), dtype=torch.float32, device=kinfo.device)
        _native.check(_native.load().virnet_kernel_from_kinfo(_native.ptr(src), len(src), k_size, sf, int(bool(shift)), _native.ptr(out),
                                                              _native.stream_handle()), "preview.kernel_from_kinfo")
    return out


def to_host(grids_u8: Sequence[Tensor]) -> List[np.ndarray]:
    """All grids of one event on the host, as uint8 arrays of their shapes: ONE copy into pinned memory and ONE event wait.  Grids that
    :func:`grids` laid into one buffer are copied as they lie; others are first gathered into one buffer on the device."""
    gs = list(grids_u8)
    if not gs:
        return []
    for g in gs:
        if not isinstance(g, Tensor) or not g.is_cuda or g.dtype != torch.uint8 or not g.is_contiguous() or g.device != gs[0].device:
            raise TypeError("preview.to_host: contiguous uint8 CUDA tensors on one device are expected")
    sizes = [g.numel() for g in gs]
    total = sum(sizes)
    with torch.no_grad(), torch.cuda.device(gs[0].device):
        store = gs[0].untyped_storage()
        adjacent = all(g.untyped_storage().data_ptr() == store.data_ptr() for g in gs) and \
            all(a.data_ptr() + n == b.data_ptr() for a, n, b in zip(gs, sizes, gs[1:]))
        flat = gs[0].as_strided((total,), (1,)) if adjacent else torch.cat([g.reshape(-1) for g in gs])
        with _native.capture_lock:                                     # (pinned allocation: not while a stream of the process captures)
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host.copy_(flat, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
    arr, out, at = host.numpy(), [], 0
    for g, n in zip(gs, sizes):
        out.append(arr[at:at + n].reshape(tuple(g.shape)))
        at += n
    return out


# ---- the events of the training scripts ------------------------------------------------------------------------------------------------------
DENOISE_TRAIN_TAGS = ("Denoised images", "GroundTruth", "Predict Sigma", "Groundtruth Sigma", "Noisy Image")
DENOISE_TEST_TAGS = ("Denoised images", "GroundTruth", "Predict Sigma", "Noise Image")
SISR_TRAIN_TAGS = ("Recover Image", "HR Image", "GT Blur Kernel", "LR Image", "Est Blur Kernel Resample", "Est Blur Kernel")
SISR_TEST_TAGS = ("Recover images", "HR Image", "LR Image", "GT Blur Kernel", "Est Blur Kernel")


def _first(mu):
    return mu[0] if isinstance(mu, (list, tuple)) else mu


def denoise_train(keep: Dict[str, Tensor], phase: str = "train") -> Tuple[List[str], List[Tensor]]:
    """train_denoising_syn.py:191-192, 201-211 from the tensors ``fit.train_step(..., keep=keep)`` left: the denoised batch (the first
    channels of ``mu`` that the ground truth has, clamped to [0, 1] as it is loaded), the ground truth, the predicted and the prior
    variance map, the noisy batch -> (tags, grids)."""
    chn = keep["im_gt"].shape[1]
    specs = [dict(x=_first(keep["mu"]), clamp=(0.0, 1.0), channels=chn), dict(x=keep["im_gt"]), dict(x=keep["sigma"]), dict(x=keep["sigma_gt"]),
             dict(x=keep["im_noisy"])]
    return [f"{phase} {t}" for t in DENOISE_TRAIN_TAGS], grids(specs)


def denoise_test(mu: Tensor, im_gt: Tensor, sigma: Tensor, im_noisy: Tensor, phase: str = "test") -> Tuple[List[str], List[Tensor]]:
    """train_denoising_syn.py:231-232, 243-250 for the batch the test loader gives (one image, [1, C, H, W] views are fine)."""
    chn = im_gt.shape[1]
    specs = [dict(x=_first(mu), clamp=(0.0, 1.0), channels=chn), dict(x=im_gt), dict(x=sigma), dict(x=im_noisy)]
    return [f"{phase} {t}" for t in DENOISE_TEST_TAGS], grids(specs)


def sisr_train(keep: Dict[str, Tensor], c: dict, phase: str = "train") -> Tuple[List[str], List[Tensor]]:
    """train_SISR.py:237, 246-263 from the tensors ``fit.sisr_train_step(..., keep=keep)`` left; ``c``: the loop's config (``k_size``,
    ``sf``, ``kernel_shift``).  As in the reference the ground-truth kernel is drawn without the shift, the estimated one with the
    config's."""
    k_gt = kernel_from_kinfo(keep["kinfo_gt"], c["k_size"], c["sf"], False)
    k_est = kernel_from_kinfo(keep["kinfo_est"], c["k_size"], c["sf"], c["kernel_shift"])
    specs = [dict(x=_first(keep["mu"])), dict(x=keep["im_hr"]), dict(x=k_gt), dict(x=keep["im_lr"]), dict(x=keep["kernel_resample"]), dict(x=k_est)]
    return [f"{phase} {t}" for t in SISR_TRAIN_TAGS], grids(specs)


def sisr_test(mu: Tensor, im_hr: Tensor, im_lr: Tensor, kinfo_gt: Tensor, kinfo_est: Tensor, c: dict, noise_type: str) -> Tuple[List[str], List[Tensor]]:
    """train_SISR.py:295-312 for one test batch of noise type ``noise_type``; both kernels with the config's shift."""
    k_gt = kernel_from_kinfo(kinfo_gt, c["k_size"], c["sf"], c["kernel_shift"])
    k_est = kernel_from_kinfo(kinfo_est, c["k_size"], c["sf"], c["kernel_shift"])
    specs = [dict(x=_first(mu)), dict(x=im_hr), dict(x=im_lr), dict(x=k_gt), dict(x=k_est)]
    return [f"Test {noise_type} {t}" for t in SISR_TEST_TAGS], grids(specs)


# ---- a writer without tensorboard ------------------------------------------------------------------------------------------------------------
class FolderWriter:
    """``add_image`` writes ``<dir>/images/<tag, spaces as _>/<step:06d>.png``, ``add_scalar`` appends ``{"tag", "value", "step"}`` as one
    JSON line to ``<dir>/scalars.jsonl``."""

    def __init__(self, directory):
        self.dir = os.fspath(directory)
        os.makedirs(os.path.join(self.dir, "images"), exist_ok=True)
        self._scalars = open(os.path.join(self.dir, "scalars.jsonl"), "a")

    def add_scalar(self, tag: str, value, step: int) -> None:
        self._scalars.write(json.dumps({"tag": str(tag), "value": float(value), "step": int(step)}) + "\n")
        self._scalars.flush()

    def add_image(self, tag: str, image, step: int, dataformats: str = "HWC") -> None:
        from PIL import Image
        image = np.asarray(image)
        if dataformats != "HWC" or image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise TypeError(f"FolderWriter.add_image takes a uint8 [H, W, 3] array with dataformats='HWC', got {image.dtype} {image.shape} {dataformats!r}")
        folder = os.path.join(self.dir, "images", str(tag).replace(" ", "_"))
        os.makedirs(folder, exist_ok=True)
        Image.fromarray(np.ascontiguousarray(image), "RGB").save(os.path.join(folder, f"{int(step):06d}.png"))

    def close(self) -> None:
        if not self._scalars.closed:
            self._scalars.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
