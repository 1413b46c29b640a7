"""The 8-way flip / rotation self-ensemble of the real-noise evaluation on the device (csrc/ensemble.hip).

The reference's SIDD and DND scripts run with ``--flip`` by default (scripts/denoising_virnet_real_sidd.py:113-154,
dnd_submission_py/pytorch_wrapper.py:15-47): every block goes through the eight symmetries of the square, each orientation is restored
in a forward of its own, the eight results are turned back, averaged, clipped and (SIDD) quantised.  ``eval.flip_ensemble`` is that loop
on the host.  Here the eight orientations of ``B`` blocks are ONE launch (:func:`expand`), the network sees them as a batch of 8 B
(square blocks) or two batches of 4 B, and the inverse, the mean, the clip and the quantisation are ONE launch (:func:`reduce`).

Orientation ``m`` is ``eval.dihedral(im, m)``.  Modes 0, 1, 4, 5 keep ``H x W`` and modes 2, 3, 6, 7 give ``W x H``, so the orientations
live in two float32 NCHW groups, ``even [4B,C,H,W]`` and ``odd [4B,C,W,H]``; the image index inside a group is ``b * 4 + j`` with ``j``
the position of the mode in :data:`EVEN_MODES` / :data:`ODD_MODES`.

The definitions are ``expand_np`` / ``reduce_np`` / ``restore_np`` below, written with ``eval.dihedral`` / ``dihedral_inverse`` and the
scripts' own expressions; the kernels give the same bits:

  * uint8 sources become ``np.float32(u / 255.0)`` -- skimage's ``img_as_float`` (a float64 division) followed by
    ``.type(torch.float32)`` -- which is NOT ``eval.img_as_float32`` (a float32 multiply by 1/255; the two differ on 126 byte values);
    float32 sources (DND) pass through;
  * ``order="sequential"`` is the SIDD script's ``acc = zeros; acc += inv_m (m = 0..7); acc /= 8`` in float32,
    ``order="pairwise"`` the DND wrapper's ``stack.mean(axis=3)``, which numpy evaluates as
    ``0 + (((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)))`` before the division;
  * ``out="uint8"`` is ``eval.img_as_ubyte(clip(.))`` (the arithmetic of ``metrics.to_uint8``), ``out="float32"`` is ``np.clip(., 0, 1)``.

Nothing here synchronises: the calls enqueue on the current stream and return device tensors, and both are safe inside a graph capture.
Results are bitwise reproducible and do not depend on where an image sits in the batch.  CPU tensors raise (no fallback).
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _native
from . import eval as veval

EVEN_MODES = (0, 1, 4, 5)      # orientations that keep H x W
ODD_MODES = (2, 3, 6, 7)       # orientations that give W x H
ORDERS = ("sequential", "pairwise")
OUTS = ("uint8", "float32")
LAYOUTS = ("hwc", "chw")


class Orientations(tuple):
    """``(even, odd)`` as :func:`expand` returns them.  ``batch``: the one ``[8B,C,H,H]`` tensor both are views of (square images), the
    ``[B,C,H,W]`` tensor itself without flip, else None."""

    def __new__(cls, even, odd, batch=None):
        self = super().__new__(cls, (even, odd))
        self.batch = batch
        return self

    even = property(lambda self: self[0])
    odd = property(lambda self: self[1])


def _options(order: str, out: str, layout: str) -> None:
    if order not in ORDERS:
        raise ValueError(f"order {order!r}: expected one of {ORDERS}")
    if out not in OUTS:
        raise ValueError(f"out {out!r}: expected one of {OUTS}")
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: expected one of {LAYOUTS}")


def _source_shape(shape, dtype_ok: bool, dtype) -> Tuple[int, int, int, int]:
    if len(shape) != 4:
        raise ValueError(f"images must be [B,H,W,C], got {tuple(shape)}")
    if not dtype_ok:
        raise TypeError(f"images must be uint8 or float32, got {dtype}")
    b, h, w, c = (int(s) for s in shape)
    if c not in (1, 3):
        raise ValueError(f"images have {c} channels, 1 or 3 expected")
    if b < 1 or h < 1 or w < 1:
        raise ValueError(f"empty images {tuple(shape)}")
    return b, h, w, c


def _group_shapes(even, odd, dtype_ok) -> Tuple[int, int, int, int, int]:
    """(B, C, H, W, modes) of a pair of orientation groups (``odd`` None: no flip)."""
    for name, t in (("even", even), ("odd", odd)):
        if t is None and name == "odd":
            continue
        if len(getattr(t, "shape", ())) != 4:
            raise ValueError(f"{name} must be [N,C,H,W], got {tuple(getattr(t, 'shape', ()))}")
        if not dtype_ok(t):
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    n, c, h, w = (int(s) for s in even.shape)
    if c not in (1, 3):
        raise ValueError(f"even has {c} channels, 1 or 3 expected")
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"empty group {tuple(even.shape)}")
    if odd is None:
        return n, c, h, w, 1
    if n % 4:
        raise ValueError(f"even holds {n} images: four orientations per source expected")
    if tuple(int(s) for s in odd.shape) != (n, c, w, h):
        raise ValueError(f"odd is {tuple(odd.shape)}, even {tuple(even.shape)} needs {(n, c, w, h)}")
    return n // 4, c, h, w, 8


# ---- definitions on the host -----------------------------------------------------------------------------------------------------------
def _as_unit_np(im: np.ndarray) -> np.ndarray:
    """One HWC image as the scripts feed it: ``img_as_float`` (float64 division) then float32 for uint8, float32 as it is."""
    return (im / 255.0).astype(np.float32) if im.dtype == np.uint8 else im


def expand_np(images: np.ndarray, flip: bool = True):
    """``(even, odd)`` as float32 NCHW arrays: orientation ``m`` of image ``b`` is ``eval.dihedral(unit(images[b]), m)`` transposed to CHW.
    Without ``flip``: ``(images as [B,C,H,W], None)``."""
    images = np.asarray(images)
    b, h, w, c = _source_shape(images.shape, images.dtype in (np.uint8, np.float32), images.dtype)
    if not flip:
        return np.stack([np.ascontiguousarray(_as_unit_np(images[i]).transpose(2, 0, 1)) for i in range(b)]), None
    groups = []
    for modes in (EVEN_MODES, ODD_MODES):
        groups.append(np.stack([np.ascontiguousarray(_as_unit_np(veval.dihedral(images[i], m)).transpose(2, 0, 1))
                                for i in range(b) for m in modes]))
    return groups[0], groups[1]


def _finish_np(mean_hwc: np.ndarray, out: str, layout: str) -> np.ndarray:
    res = veval.img_as_ubyte(mean_hwc.clip(0, 1)) if out == "uint8" else np.clip(mean_hwc, 0.0, 1.0)
    return np.ascontiguousarray(res.transpose(2, 0, 1)) if layout == "chw" else res


def reduce_np(even: np.ndarray, odd: Optional[np.ndarray], order: str = "sequential", out: str = "uint8", layout: str = "hwc") -> np.ndarray:
    """The restored orientation groups back to one image per source, by the scripts' expressions."""
    _options(order, out, layout)
    b, c, h, w, modes = _group_shapes(even, odd, lambda a: a.dtype == np.float32)
    res = []
    for i in range(b):
        if modes == 1:
            res.append(_finish_np(even[i].transpose(1, 2, 0), out, layout))
            continue
        back = {}
        for group, ms in ((even, EVEN_MODES), (odd, ODD_MODES)):
            for j, m in enumerate(ms):
                back[m] = veval.dihedral_inverse(group[i * 4 + j].transpose(1, 2, 0), m)
        if order == "sequential":                      # scripts/denoising_virnet_real_sidd.py:121-136
            mean = np.zeros((h, w, c), dtype=np.float32)
            for m in range(8):
                mean += back[m]
            mean /= 8
        else:                                          # dnd_submission_py/pytorch_wrapper.py:19-33
            stack = np.zeros((h, w, c, 8), dtype=np.float32)
            for m in range(8):
                stack[:, :, :, m] = back[m]
            mean = stack.mean(axis=3, keepdims=False)
        res.append(_finish_np(mean, out, layout))
    return np.stack(res)


def _chunks(n: int, batch: int):
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"batch {batch}: at least 1")
    return [(a, min(a + batch, n)) for a in range(0, n, batch)]


def restore_np(forward: Callable[[np.ndarray], np.ndarray], images: np.ndarray, flip: bool = True, order: str = "sequential",
               out: str = "uint8", layout: str = "hwc", batch: int = 8) -> np.ndarray:
    """:func:`restore` on the host: ``forward`` maps a float32 ``[n,C,h,w]`` array to one of the same shape."""
    even, odd = expand_np(images, flip)
    run = lambda g: np.concatenate([np.asarray(forward(g[a:b]), dtype=np.float32) for a, b in _chunks(len(g), batch)])   # noqa: E731
    return reduce_np(run(even), None if odd is None else run(odd), order, out, layout)


# ---- the device path -------------------------------------------------------------------------------------------------------------------
def _device_source(images) -> Tensor:
    if isinstance(images, np.ndarray):
        _source_shape(images.shape, images.dtype in (np.uint8, np.float32), images.dtype)
        if not torch.cuda.is_available():
            raise RuntimeError("no ROCm device: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
        host = np.ascontiguousarray(images) if images.flags.writeable else np.array(images)      # (torch refuses read-only memory)
        return torch.from_numpy(host).to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
    if not isinstance(images, Tensor):
        raise TypeError(f"images must be a numpy array or a CUDA tensor, got {type(images).__name__}")
    _source_shape(images.shape, images.dtype in (torch.uint8, torch.float32), images.dtype)
    if not images.is_cuda:
        raise RuntimeError(f"images is on {images.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    return images.detach().contiguous()


def expand(images, flip: bool = True) -> Orientations:
    """The eight orientations of ``B`` images in one launch.  ``images``: uint8 or float32 ``[B,H,W,C]`` (C 1 or 3), a numpy array
    (uploaded once) or a CUDA tensor.  Returns ``(even [4B,C,H,W], odd [4B,C,W,H])`` float32; for square images they are the two halves of
    one ``[8B,C,H,H]`` tensor, ``.batch``, so that the forward sees one batch and nothing is concatenated.  ``flip=False``:
    ``(images as float32 [B,C,H,W], None)``."""
    src = _device_source(images)
    b, h, w, c = src.shape
    modes = 8 if flip else 1
    with torch.cuda.device(src.device):
        if not flip:
            whole = even = torch.empty((b, c, h, w), dtype=torch.float32, device=src.device)
            odd = None
        elif h == w:
            whole = torch.empty((8 * b, c, h, w), dtype=torch.float32, device=src.device)
            even, odd = whole[:4 * b], whole[4 * b:]
        else:
            whole = None
            even = torch.empty((4 * b, c, h, w), dtype=torch.float32, device=src.device)
            odd = torch.empty((4 * b, c, w, h), dtype=torch.float32, device=src.device)
        _native.check(_native.load().virnet_ensemble_expand(src.data_ptr(), int(src.dtype == torch.float32), even.data_ptr(), _native.ptr(odd),
                                                            b, h, w, c, modes, _native.stream_handle()), "ensemble_expand")
    return Orientations(even, odd, whole)


def reduce(even: Tensor, odd: Optional[Tensor], order: str = "sequential", out: str = "uint8", layout: str = "hwc") -> Tensor:
    """The inverse of :func:`expand` on the restored groups in one launch: every orientation turned back, the eight averaged in float32 in
    the given ``order``, clipped to [0,1] and, for ``out="uint8"``, quantised.  Returns ``[B,H,W,C]`` (``"hwc"``, what the scripts store)
    or ``[B,C,H,W]`` (``"chw"``, what ``metrics.psnr_ssim`` takes).  ``odd=None``: no flip -- clip, quantisation and layout change only."""
    _options(order, out, layout)
    for name, t in (("even", even), ("odd", odd)):
        if t is not None and not isinstance(t, Tensor):
            raise TypeError(f"{name} must be a CUDA tensor, got {type(t).__name__}")
    b, c, h, w, modes = _group_shapes(even, odd, lambda t: t.dtype == torch.float32)
    for name, t in (("even", even), ("odd", odd)):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    if odd is not None and odd.device != even.device:
        raise RuntimeError(f"even is on {even.device}, odd on {odd.device}")
    even = even.detach().contiguous()
    odd = None if odd is None else odd.detach().contiguous()
    with torch.cuda.device(even.device):
        res = torch.empty((b, h, w, c) if layout == "hwc" else (b, c, h, w), dtype=torch.uint8 if out == "uint8" else torch.float32,
                          device=even.device)
        _native.check(_native.load().virnet_ensemble_reduce(even.data_ptr(), _native.ptr(odd), res.data_ptr(), int(out == "float32"),
                                                            int(order == "pairwise"), int(layout == "chw"), b, h, w, c, modes,
                                                            _native.stream_handle()), "ensemble_reduce")
    return res


def _run_group(forward: Callable[[Tensor], Tensor], x: Tensor, batch: int) -> Tensor:
    """``forward`` over ``x`` in chunks of at most ``batch`` images; one chunk's result is used as it is."""
    res = None
    for a, b in _chunks(x.shape[0], batch):
        y = forward(x[a:b])
        if not isinstance(y, Tensor) or not y.is_cuda or y.dtype != torch.float32 or y.shape != x[a:b].shape:
            raise ValueError(f"forward must map a float32 CUDA tensor {tuple(x[a:b].shape)} to one of the same shape, got "
                             f"{tuple(getattr(y, 'shape', ()))} {getattr(y, 'dtype', type(y).__name__)}")
        if (a, b) == (0, x.shape[0]):
            return y
        if res is None:
            res = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        res[a:b].copy_(y)
    return res


def restored_groups(forward: Callable[[Tensor], Tensor], groups: Orientations, batch: int = 8) -> Tuple[Tensor, Optional[Tensor]]:
    """``forward`` on the orientation batches of :func:`expand` in chunks of at most ``batch`` images: the ``(even, odd)`` that
    :func:`reduce` takes.  Square images run as ONE sequence of chunks over the ``[8B,...]`` tensor."""
    even, odd = groups
    if odd is None:
        return _run_group(forward, even, batch), None
    if groups.batch is not None:
        y = _run_group(forward, groups.batch, batch)
        return y[:even.shape[0]], y[even.shape[0]:]
    return _run_group(forward, even, batch), _run_group(forward, odd, batch)


def restore(forward: Callable[[Tensor], Tensor], images, flip: bool = True, order: str = "sequential", out: str = "uint8",
            layout: str = "hwc", batch: int = 8) -> Tensor:
    """The scripts' self-ensemble around any ``forward: [n,C,h,w] -> [n,C,h,w]`` (e.g. ``lambda x: net(x)[0]``): :func:`expand`, ``forward``
    on the orientation batches in chunks of at most ``batch`` images, :func:`reduce`.  Never synchronises; returns a CUDA tensor."""
    _options(order, out, layout)
    return reduce(*restored_groups(forward, expand(images, flip), batch), order=order, out=out, layout=layout)
