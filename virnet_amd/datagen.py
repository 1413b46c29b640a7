"""Training batches synthesised on the device from a device-resident uint8 image pool (csrc/datagen.hip).

What the reference's dataset classes do per sample on the host -- crop, float conversion, sigma map, ``torch.randn``, eight-way augmentation,
blur-kernel construction, three host-to-device copies (datasets/DenoisingDatasets.py:74-99, 137-155, 190-253, datasets/SISRDatasets.py:66-122,
train_denoising_syn.py:171) -- as one launch per batch:

  * :class:`ImagePool`          -- the decoded training images, uploaded once: one uint8 buffer (HWC, back to back) and a table;
  * :func:`draw_denoise_params`, :func:`draw_pair_params`, :func:`draw_sisr_params` -- the per-sample random parameters, drawn on the host
    from a ``random.Random`` in the reference's order (a seeded single-worker reference dataset and these, seeded alike, agree);
  * :func:`denoise_batch`       -- ``SimulateTrain.__getitem__`` collated: (im_noisy, im_gt, sigma_map_gt);
  * :func:`pair_batch`          -- ``RealTrain`` / ``DataLMDB``: (im_noisy, im_gt);
  * :func:`draw_mixup_params`, :func:`mixup`, :func:`real_batch` -- ``MixUp_AUG.aug`` (datasets/data_tools.py:12-30) and the batch of the
    real-noise loop (train_denoising_real.py:160-164): paired patches, mixed, with the variance prior ``sigma_gt``;
  * :func:`hr_batch`, :func:`blur_kernels`, :func:`normal`, :func:`sisr_batch` -- ``GeneralTrainFloder.__getitem__`` collated, ending in the
    existing ``degrade.synthesize_lr``;
  * :class:`SimulateTestSet` -- ``SimulateTest`` (datasets/DenoisingDatasets.py:255-296), the validation set of the synthetic-noise
    training: one noise array and one sigma map for the whole set, uploaded once; a batch of same-shape images is one launch;
  * :class:`GeneralTestSet` -- ``GeneralTest`` (datasets/SISRDatasets.py:124-207), the validation set of the SISR training: every image
    degraded once at construction with the device operators and kept resident; a batch is a view.

Every device function has its definition in numpy beside it (``*_np``): that is the specification, pinned to batches the reference's own
classes produced (tests/golden/datagen.npz); the kernels are tested against it.

CUDA tensors only, no fallback.  Nothing here synchronises: a call uploads its parameters in one pinned non-blocking copy (or takes
:class:`DeviceParams` that are already there) and enqueues on the current stream of the pool's device.  Results are bitwise reproducible and a
sample's values do not depend on its position in the batch.  Image decoding stays with the caller (``eval.imread_rgb_uint8``); the
reference's ``cv2.resize`` of images smaller than the patch is not reproduced -- such a pool is refused.
"""
from __future__ import annotations

import functools
import math
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _native, degrade, sisr_eval
from . import eval as veval

MAX_PATCH = _native.DATAGEN_MAX_PATCH
MAX_KERNEL = _native.DATAGEN_MAX_KERNEL
SIMTEST_MAP = _native.SIMTEST_MAP
DENOISE, PAIR, HR = 0, 1, 2
STREAM_DENOISE, STREAM_SISR_LR = 0, 1          # the generator's ``stream`` word: one per use, so that no two uses share normals
RECORD_BYTES = 96
_I32 = ("img", "ind_h", "ind_w", "flag", "niid", "qf")                                    # int32 sections 0..5; 6: std as fp32; 7: unused
_F64 = ("center_h", "center_w", "denom", "down", "up", "lam1_sq", "lam2_sq", "theta")      # fp64 sections


# ---- the pool -------------------------------------------------------------------------------------------------------------------------------
def _check_images(images, what: str) -> List[np.ndarray]:
    images = list(images)
    if not images:
        raise ValueError(f"{what}: an empty list of images")
    for i, im in enumerate(images):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise TypeError(f"{what}: image {i} must be a uint8 [H,W,3] array, got "
                            f"{type(im).__name__} {getattr(im, 'dtype', '')} {getattr(im, 'shape', '')}")
    return images


def _require_device(device, who: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: device {dev}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class ImagePool:
    """``ImagePool(images, device)``: a list of uint8 [H,W,3] RGB arrays of differing sizes as one uint8 device buffer ``data`` (HWC, images
    back to back, no padding) and ``table`` (device int64 [M,3]: byte offset, height, width), uploaded once.  ``shapes`` keeps the (H, W)
    pairs on the host for the parameter drawers.  :meth:`paired` adds a second buffer ``data_b`` of pairwise equal shapes (the real-noise
    datasets: noisy in ``data``, ground truth in ``data_b``).  A pool may be built on the CPU (to draw parameters, or for the ``*_np``
    definitions); the batch entry points refuse it."""

    def __init__(self, images: Sequence[np.ndarray], device, _second: Optional[Sequence[np.ndarray]] = None):
        images = _check_images(images, "ImagePool")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.shapes: List[Tuple[int, int]] = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        sizes = [h * w * 3 for h, w in self.shapes]
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        table = np.stack([offsets, np.asarray([s[0] for s in self.shapes], dtype=np.int64), np.asarray([s[1] for s in self.shapes], dtype=np.int64)], 1)
        self.device = dev
        with _native.capture_lock:
            self.data: Tensor = torch.from_numpy(np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])).to(dev)
            self.table: Tensor = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
            self.data_b: Optional[Tensor] = None
            if _second is not None:
                self.data_b = torch.from_numpy(np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in _second])).to(dev)

    @classmethod
    def paired(cls, noisy: Sequence[np.ndarray], gt: Sequence[np.ndarray], device) -> "ImagePool":
        noisy, gt = _check_images(noisy, "ImagePool.paired (noisy)"), _check_images(gt, "ImagePool.paired (gt)")
        if len(noisy) != len(gt):
            raise ValueError(f"ImagePool.paired: {len(noisy)} noisy images but {len(gt)} ground-truth images")
        for i, (a, b) in enumerate(zip(noisy, gt)):
            if a.shape != b.shape:
                raise ValueError(f"ImagePool.paired: pair {i} has shapes {a.shape} and {b.shape}")
        return cls(noisy, device, _second=gt)

    def __len__(self) -> int:
        return len(self.shapes)


def _pool_shapes(pool) -> List[Tuple[int, int]]:
    """(H, W) per image of an ImagePool, or of a plain list of shapes / arrays (the host definitions need no device)."""
    if isinstance(pool, ImagePool):
        return pool.shapes
    return [(int(s.shape[0]), int(s.shape[1])) if isinstance(s, np.ndarray) else (int(s[0]), int(s[1])) for s in pool]


def _check_patch(shapes, pch_size: int) -> int:
    """The patch size, once every image of the pool is known to hold it."""
    if isinstance(pch_size, bool) or int(pch_size) != pch_size or not 1 <= int(pch_size) <= MAX_PATCH:
        raise ValueError(f"patch size {pch_size!r}: an integer 1..{MAX_PATCH} is expected")
    p = int(pch_size)
    for i, (h, w) in enumerate(shapes):
        if h < p or w < p:
            raise ValueError(f"image {i} is {h}x{w}, smaller than the {p}x{p} patch: the reference's cv2.resize of undersized images "
                             f"(BaseDataSetImg.crop_patch) is out of scope here; resize or drop it before building the pool")
    return p


# ---- the parameters of a batch (host) -------------------------------------------------------------------------------------------------------
class BatchParams:
    """The random parameters of ``n`` samples as small numpy arrays, all [n]: ``img``, ``ind_h``, ``ind_w``, ``flag`` (int32: image index,
    crop origin, augmentation 0..7); for the denoiser ``niid`` (int32 0/1), ``center_h``, ``center_w``, ``scale``, ``up``, ``down`` (fp64; iid
    samples keep their level in ``down``); for SISR ``lam1``, ``lam2``, ``theta`` (fp64), ``std`` (fp64, already divided by 255) and ``qf``
    (int32, 0: no JPEG).  Fields a mode does not use keep a harmless default.  Ranges are checked against ``shapes`` on construction: every
    crop must lie inside the image it names (the drawers, which may pick any image, demand that of the whole pool)."""

    def __init__(self, shapes, pch_size: int, img, ind_h, ind_w, flag, **fields):
        self.shapes = _pool_shapes(shapes)
        if isinstance(pch_size, bool) or int(pch_size) != pch_size or not 1 <= int(pch_size) <= MAX_PATCH:
            raise ValueError(f"patch size {pch_size!r}: an integer 1..{MAX_PATCH} is expected")
        self.pch_size = int(pch_size)
        self.img, self.ind_h, self.ind_w, self.flag = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (img, ind_h, ind_w, flag))
        n = self.n = int(self.img.shape[0])
        if n < 1 or n > 65535:
            raise ValueError(f"{n} samples (1..65535 expected)")
        for name in ("niid", "qf"):
            setattr(self, name, np.asarray(fields.pop(name, np.zeros(n)), dtype=np.int64).reshape(-1))
        for name, default in (("center_h", 0.0), ("center_w", 0.0), ("scale", 1.0), ("up", 0.0), ("down", 0.0), ("lam1", 1.0), ("lam2", 1.0),
                              ("theta", 0.0), ("std", 0.0)):
            setattr(self, name, np.asarray(fields.pop(name, np.full(n, default)), dtype=np.float64).reshape(-1))
        if fields:
            raise TypeError(f"unknown parameter fields {sorted(fields)}")
        self.validate()
        for name in ("img", "ind_h", "ind_w", "flag", "niid", "qf"):
            setattr(self, name, getattr(self, name).astype(np.int32))

    def validate(self) -> None:
        n, p = self.n, self.pch_size
        for name in ("ind_h", "ind_w", "flag", "niid", "qf", "center_h", "center_w", "scale", "up", "down", "lam1", "lam2", "theta", "std"):
            if getattr(self, name).shape != (n,):
                raise ValueError(f"{name} has shape {getattr(self, name).shape}, ({n},) expected")
        for i in range(n):
            if not 0 <= self.img[i] < len(self.shapes):
                raise ValueError(f"sample {i}: image index {self.img[i]} outside 0..{len(self.shapes) - 1}")
            h, w = self.shapes[int(self.img[i])]
            if not 0 <= self.ind_h[i] <= h - p or not 0 <= self.ind_w[i] <= w - p:
                raise ValueError(f"sample {i}: a {p}x{p} crop at ({self.ind_h[i]}, {self.ind_w[i]}) runs past the edge of its {h}x{w} image")
            if not 0 <= self.flag[i] <= 7:
                raise ValueError(f"sample {i}: augmentation flag {self.flag[i]} outside 0..7")
            if not 0 <= self.qf[i] <= 100:
                raise ValueError(f"sample {i}: JPEG quality {self.qf[i]} outside 0..100")
        floats = np.stack([self.center_h, self.center_w, self.scale, self.up, self.down, self.lam1, self.lam2, self.theta, self.std])
        if not np.isfinite(floats).all():
            raise ValueError("a non-finite parameter")
        if (self.scale <= 0).any() or (self.lam1 <= 0).any() or (self.lam2 <= 0).any() or (self.std < 0).any():
            raise ValueError("scale, lam1 and lam2 must be positive and std non-negative")
        if ((self.niid != 0) & ((self.center_h < 0) | (self.center_h > p) | (self.center_w < 0) | (self.center_w > p))).any():
            raise ValueError(f"a sigma-map centre outside [0, {p}]")

    def select(self, index) -> "BatchParams":
        """The samples ``index`` (anything numpy takes as a 1-D index) as parameters of their own."""
        idx = np.arange(self.n)[index]
        kw = {k: getattr(self, k)[idx] for k in ("niid", "qf", "center_h", "center_w", "scale", "up", "down", "lam1", "lam2", "theta", "std")}
        return BatchParams(self.shapes, self.pch_size, self.img[idx], self.ind_h[idx], self.ind_w[idx], self.flag[idx], **kw)

    def pack(self) -> np.ndarray:
        """The device blob (include/virnet_hip.h): uint8 [96 n], eight 4-byte sections then eight fp64 sections of n values each."""
        n = self.n
        blob = np.zeros(RECORD_BYTES * n, dtype=np.uint8)
        i32, f32, f64 = blob[:32 * n].view(np.int32), blob[:32 * n].view(np.float32), blob[32 * n:].view(np.float64)
        for s, name in enumerate(_I32):
            i32[s * n:(s + 1) * n] = getattr(self, name)
        f32[6 * n:7 * n] = self.std.astype(np.float32)
        cols = dict(center_h=self.center_h, center_w=self.center_w, denom=np.asarray([2 * float(s) ** 2 for s in self.scale]), down=self.down,
                    up=self.up, lam1_sq=self.lam1 ** 2, lam2_sq=self.lam2 ** 2, theta=self.theta)
        for s, name in enumerate(_F64):
            f64[s * n:(s + 1) * n] = cols[name]
        return blob

    def to(self, device) -> "DeviceParams":
        return DeviceParams(self, device)


class DeviceParams:
    """:class:`BatchParams` on the device: ``blob`` (uint8 [96 n]) with views of its sections (``std`` fp32 [n], ``qf`` int32 [n], ``lam1_sq``,
    ``lam2_sq``, ``theta`` fp64 [n]).  :meth:`update` overwrites the same buffer with other parameters of the same size -- what a captured
    graph replays against."""

    def __init__(self, params: BatchParams, device):
        dev = _require_device(device, "DeviceParams")
        self.n, self.pch_size, self.shapes = params.n, params.pch_size, params.shapes
        self.blob = torch.empty(RECORD_BYTES * self.n, dtype=torch.uint8, device=dev)
        self.update(params)

    def update(self, params: BatchParams) -> "DeviceParams":
        if params.n != self.n or params.pch_size != self.pch_size or params.shapes != self.shapes:
            raise ValueError("DeviceParams.update: the parameters are of another batch size, patch size or pool")
        with _native.capture_lock:      # (pinned allocation is not permitted while any stream of the process captures)
            staged = torch.empty(RECORD_BYTES * self.n, dtype=torch.uint8, pin_memory=True)
        staged.numpy()[:] = params.pack()
        self.blob.copy_(staged, non_blocking=True)
        self.any_qf = bool((params.qf != 0).any())
        return self

    def _section(self, byte0: int, dtype) -> Tensor:
        size = 8 if dtype == torch.float64 else 4
        return self.blob[byte0:byte0 + size * self.n].view(dtype)

    @property
    def qf(self) -> Tensor:
        return self._section(4 * 5 * self.n, torch.int32)

    @property
    def std(self) -> Tensor:
        return self._section(4 * 6 * self.n, torch.float32)

    @property
    def lam1_sq(self) -> Tensor:
        return self._section((32 + 8 * 5) * self.n, torch.float64)

    @property
    def lam2_sq(self) -> Tensor:
        return self._section((32 + 8 * 6) * self.n, torch.float64)

    @property
    def theta(self) -> Tensor:
        return self._section((32 + 8 * 7) * self.n, torch.float64)


class MixParams:
    """The mix of one batch of ``n`` samples (``MixUp_AUG.aug``, datasets/data_tools.py:19-30): ``perm`` (int32 [n], each 0..n-1: sample i is
    mixed with sample ``perm[i]``; the drawer gives a permutation, repeated indices are accepted since the kernels only read through them)
    and ``lam`` (fp32 [n], finite, in [0, 1]: the weight of the sample itself).  Checked on construction; the device trusts it."""

    def __init__(self, perm, lam):
        perm = np.asarray(perm.detach().cpu() if isinstance(perm, Tensor) else perm)
        if perm.dtype.kind not in "iu":
            raise TypeError(f"perm must hold integers, got {perm.dtype}")
        self.perm = perm.astype(np.int64).reshape(-1)
        self.lam = np.asarray(lam.detach().cpu() if isinstance(lam, Tensor) else lam, dtype=np.float32).reshape(-1)
        self.n = int(self.perm.shape[0])
        self.validate()
        self.perm = self.perm.astype(np.int32)

    def validate(self) -> None:
        n = int(self.perm.shape[0])
        if self.lam.shape != (n,):
            raise ValueError(f"perm has {n} entries but lam has {self.lam.shape[0]}")
        if n < 1 or n > 65535:
            raise ValueError(f"perm: {n} samples (1..65535 expected)")
        for i in range(n):
            if not 0 <= self.perm[i] < n:
                raise ValueError(f"perm[{i}] = {self.perm[i]} outside 0..{n - 1}")
            if not (np.isfinite(self.lam[i]) and 0.0 <= self.lam[i] <= 1.0):
                raise ValueError(f"lam[{i}] = {self.lam[i]}: finite values in [0, 1] are expected")

    def pack(self) -> np.ndarray:
        """The device buffer (include/virnet_hip.h): uint8 [8 n] = int32 perm[n], then fp32 lam[n]."""
        blob = np.zeros(8 * self.n, dtype=np.uint8)
        blob[:4 * self.n].view(np.int32)[:] = self.perm
        blob[4 * self.n:].view(np.float32)[:] = self.lam
        return blob

    def to(self, device) -> "DeviceMix":
        return DeviceMix(self, device)


class DeviceMix:
    """:class:`MixParams` on the device: ``blob`` (uint8 [8 n]).  :meth:`update` overwrites the same buffer with another mix of the same
    size -- what a captured graph replays against -- in one pinned, non-blocking copy."""

    def __init__(self, mix: MixParams, device):
        dev = _require_device(device, "DeviceMix")
        self.n = mix.n
        self.blob = torch.empty(8 * self.n, dtype=torch.uint8, device=dev)
        self.update(mix)

    def update(self, mix: MixParams) -> "DeviceMix":
        if not isinstance(mix, MixParams) or mix.n != self.n:
            raise ValueError("DeviceMix.update: a MixParams of the same batch size is expected")
        with _native.capture_lock:      # (pinned allocation is not permitted while any stream of the process captures)
            staged = torch.empty(8 * self.n, dtype=torch.uint8, pin_memory=True)
        staged.numpy()[:] = mix.pack()
        self.blob.copy_(staged, non_blocking=True)
        return self


def draw_mixup_params(n: int, alpha: float = 0.6) -> MixParams:
    """The random part of ``MixUp_AUG.aug`` (datasets/data_tools.py:17-25) for a batch of ``n``: ``torch.randperm(n)``, then
    ``Beta(tensor([alpha]), tensor([alpha])).rsample((n, 1))``, in that order.  ``torch.distributions`` takes no generator argument, so
    torch's GLOBAL CPU generator is the interface: after ``torch.manual_seed(s)`` this returns the ``perm`` and ``lam`` the reference would
    use after the same seed, and leaves the generator where the reference leaves it."""
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= 65535:
        raise ValueError(f"{n!r} samples (an integer 1..65535 expected)")
    if not float(alpha) > 0.0:
        raise ValueError(f"alpha {alpha!r}: a positive concentration is expected")
    perm = torch.randperm(int(n))
    dist = torch.distributions.beta.Beta(torch.tensor([float(alpha)]), torch.tensor([float(alpha)]))
    lam = dist.rsample((int(n), 1))
    return MixParams(perm.numpy(), lam.reshape(-1).numpy())


def _crop(rng: random.Random, shapes, p: int) -> Tuple[int, int, int]:
    ind_im = rng.randint(0, len(shapes) - 1)
    h, w = shapes[ind_im]
    return ind_im, rng.randint(0, h - p), rng.randint(0, w - p)


def draw_denoise_params(rng: random.Random, pool, n: int, pch_size: int, mode: str = "niid", sigma_min: float = 0, sigma_max: float = 75) -> BatchParams:
    """``n`` samples of ``SimulateTrain.__getitem__`` (datasets/DenoisingDatasets.py:217-243), consuming ``rng`` in its order per sample: image
    index, ``ind_H``, ``ind_W``; niid: centre x 2, scale, ``up``, ``down`` (swapped and + 5/255 as there); iid: the level; then the
    augmentation flag."""
    shapes = _pool_shapes(pool)
    p = _check_patch(shapes, pch_size)
    mode = str(mode).lower()
    if mode not in ("niid", "iid"):
        raise ValueError("mode must be 'niid' or 'iid'")
    cols = {k: [] for k in ("img", "ind_h", "ind_w", "flag", "niid", "center_h", "center_w", "scale", "up", "down")}
    for _ in range(int(n)):
        ind_im, ind_h, ind_w = _crop(rng, shapes, p)
        if mode == "niid":
            center = [rng.uniform(0, p), rng.uniform(0, p)]
            scale = rng.uniform(p / 4, p / 4 * 3)
            up = rng.uniform(sigma_min / 255.0, sigma_max / 255.0)
            down = rng.uniform(sigma_min / 255.0, sigma_max / 255.0)
            if up < down:
                up, down = down, up
            up += 5 / 255.0
        else:
            center, scale, up = [0.0, 0.0], 1.0, 0.0
            down = rng.uniform(sigma_min / 255.0, sigma_max / 255.0)
        flag = rng.randint(0, 7)
        for k, v in zip(cols, (ind_im, ind_h, ind_w, flag, int(mode == "niid"), center[0], center[1], scale, up, down)):
            cols[k].append(v)
    return BatchParams(shapes, p, **cols)


def draw_pair_params(rng: random.Random, pool, n: int, pch_size: int) -> BatchParams:
    """``n`` samples of ``RealTrain`` / ``DataLMDB.__getitem__`` (datasets/DenoisingDatasets.py:78-93, 138-149): image index, ``ind_H``,
    ``ind_W``, augmentation flag."""
    shapes = _pool_shapes(pool)
    p = _check_patch(shapes, pch_size)
    rows = [_crop(rng, shapes, p) + (rng.randint(0, 7),) for _ in range(int(n))]
    return BatchParams(shapes, p, *(list(c) for c in zip(*rows)))


def _random_qf(rng: random.Random) -> int:
    start = list(range(30, 50, 5)) + [60, 70, 80]          # GeneralTrainFloder.random_qf (datasets/SISRDatasets.py:52-60)
    end = list(range(35, 50, 5)) + [60, 70, 80, 95]
    ind_range = rng.randint(0, len(start) - 1)
    return rng.randint(start[ind_range], end[ind_range])


def draw_sisr_params(rng: random.Random, pool, n: int, hr_size: int, sf: int, noise_level=(0.1, 15), add_jpeg: bool = False,
                     noise_jpeg=(0.1, 10)) -> BatchParams:
    """``n`` samples of ``GeneralTrainFloder.__getitem__`` (datasets/SISRDatasets.py:66-110) in its order: image index, ``ind_H``, ``ind_W``,
    augmentation flag, ``lam1``, ``random.random()`` and then ``lam2`` only when it is below 0.7, ``theta``, the ``random.sample`` over the
    noise types (which consumes the stream even when there is one type), and ``std``; a JPEG sample draws its quality before its ``std``."""
    shapes = _pool_shapes(pool)
    p = _check_patch(shapes, hr_size)
    if not noise_level[0] < noise_level[1] or not noise_jpeg[0] < noise_jpeg[1]:
        raise ValueError("noise_level and noise_jpeg must be increasing pairs")
    noise_types = ["Gaussian"] + (["JPEG"] if add_jpeg else [])
    cols = {k: [] for k in ("img", "ind_h", "ind_w", "flag", "lam1", "lam2", "theta", "std", "qf")}
    for _ in range(int(n)):
        ind_im, ind_h, ind_w = _crop(rng, shapes, p)
        flag = rng.randint(0, 7)
        lam1 = rng.uniform(0.2, sf)
        lam2 = rng.uniform(lam1, sf) if rng.random() < 0.7 else lam1
        theta = rng.uniform(0, np.pi)
        noise_type = rng.sample(noise_types, k=1)[0]
        qf = 0
        if noise_type == "Gaussian":
            std = rng.uniform(noise_level[0], noise_level[1]) / 255.0
        else:
            qf = _random_qf(rng)
            std = rng.uniform(noise_jpeg[0], noise_jpeg[1]) / 255.0
        for k, v in zip(cols, (ind_im, ind_h, ind_w, flag, lam1, lam2, theta, std, qf)):
            cols[k].append(v)
    return BatchParams(shapes, p, **cols)


# ---- the definitions in numpy ---------------------------------------------------------------------------------------------------------------
def u8_to_float_np(u8: np.ndarray, divide: bool = False) -> np.ndarray:
    """uint8 -> fp32 in [0,1]: ``u8 * fp32(1/255)`` (skimage's img_as_float32, ``eval.img_as_float32``) or, with ``divide``, ``u8 / 255`` as a
    true fp32 division (util_image.imread, utils/util_image.py:206).  The two differ in the last bit for 126 of the 256 values."""
    x = np.asarray(u8, dtype=np.uint8).astype(np.float32)
    return x / np.float32(255.0) if divide else x * np.float32(1.0 / 255.0)


def augment_np(x: np.ndarray, flag: int) -> np.ndarray:
    """util_image.data_aug_np (utils/util_image.py:391-434) on an [H,W,...] array: ``flag >> 1`` quarter turns counter-clockwise
    (``np.rot90``), then ``np.flipud`` for odd flags."""
    if not 0 <= int(flag) <= 7:
        raise ValueError(f"augmentation flag {flag} outside 0..7")
    out = np.rot90(x, k=int(flag) >> 1)
    return np.flipud(out) if int(flag) & 1 else out


def sigma_map_np(p: int, center_h: float, center_w: float, scale: float, up: float, down: float) -> np.ndarray:
    """The normalised bump of ``generate_sigma_niid`` (datasets/DenoisingDatasets.py:190-203) -> fp32 [p,p], without a reduction: the
    reference divides the bump by its sum (which cancels) and normalises by its minimum and maximum, which sit at the corner farthest from
    the centre and at the pixel nearest to it."""
    ii, jj = (x.astype(np.float64) for x in np.meshgrid(np.arange(p), np.arange(p), indexing="ij"))
    denom = 2 * float(scale) ** 2

    def bump(di2, dj2):
        return np.exp((-di2 - dj2) / denom)

    def near(c):
        i0 = min(math.floor(c), p - 1)
        i1 = min(i0 + 1, p - 1)
        return min((i0 - c) * (i0 - c), (i1 - c) * (i1 - c))

    def far(c):
        return max((0.0 - c) * (0.0 - c), (p - 1 - c) * (p - 1 - c))

    e = bump((ii - center_h) * (ii - center_h), (jj - center_w) * (jj - center_w))
    e_min, e_max = bump(far(center_h), far(center_w)), bump(near(center_h), near(center_w))
    return (down + (e - e_min) / (e_max - e_min) * (up - down)).astype(np.float32)


def _sample_sigma_np(params: BatchParams, i: int) -> np.ndarray:
    p = params.pch_size
    if params.niid[i]:
        return sigma_map_np(p, float(params.center_h[i]), float(params.center_w[i]), float(params.scale[i]), float(params.up[i]), float(params.down[i]))
    return (np.ones([p, p]) * params.down[i]).astype(np.float32)


def _crop_np(images, params: BatchParams, i: int) -> np.ndarray:
    p, y, x = params.pch_size, int(params.ind_h[i]), int(params.ind_w[i])
    return images[int(params.img[i])][y:y + p, x:x + p]


def _nchw(samples) -> np.ndarray:
    return np.ascontiguousarray(np.stack([s.transpose(2, 0, 1) for s in samples]))


def denoise_batch_np(images, params: BatchParams, noise: np.ndarray, clip: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition of :func:`denoise_batch`: ``images`` the pool's uint8 arrays, ``noise`` fp32 [N,3,P,P] standard normals at source
    coordinates -> (im_noisy, im_gt, sigma_map_gt), fp32 NCHW (datasets/DenoisingDatasets.py:217-253)."""
    noisy, gts, maps = [], [], []
    for i in range(params.n):
        im_gt = u8_to_float_np(_crop_np(images, params, i))
        sigma = _sample_sigma_np(params, i)[:, :, np.newaxis]
        nz = np.ascontiguousarray(np.asarray(noise[i], dtype=np.float32).transpose(1, 2, 0)) * sigma
        im_noisy = im_gt + nz
        if clip:
            im_noisy = np.clip(im_noisy, np.float32(0.0), np.float32(1.0))
        im_gt, im_noisy, sigma = (augment_np(x, params.flag[i]) for x in (im_gt, im_noisy, sigma))
        sq = np.square(sigma)
        maps.append(np.where(sq < np.float32(1e-10), np.float32(1e-10), sq))
        gts.append(im_gt)
        noisy.append(im_noisy)
    return _nchw(noisy), _nchw(gts), _nchw(maps)


def pair_batch_np(noisy_images, gt_images, params: BatchParams) -> Tuple[np.ndarray, np.ndarray]:
    """The definition of :func:`pair_batch` (datasets/DenoisingDatasets.py:137-155)."""
    return tuple(_nchw([augment_np(u8_to_float_np(_crop_np(ims, params, i)), params.flag[i]) for i in range(params.n)])
                 for ims in (noisy_images, gt_images))


def mixup_np(x: np.ndarray, mix: MixParams) -> np.ndarray:
    """The definition of :func:`mixup` for one tensor (datasets/data_tools.py:22-28): fp32 [N,...] -> ``lam * x + (1 - lam) * x[perm]``, all
    in fp32 with ``1 - lam``, the two products and the sum each rounded on their own, as the reference's separate torch ops round them (a
    fused multiply-add differs in the last bit on about a fifth of the elements)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim < 1 or x.shape[0] != mix.n:
        raise ValueError(f"a batch of {x.shape[0] if x.ndim else 0} samples but a mix of {mix.n}")
    lam = mix.lam.astype(np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    return lam * x + (np.float32(1) - lam) * x[mix.perm]


def real_batch_np(noisy_images, gt_images, params: BatchParams, mix: MixParams) -> Tuple[np.ndarray, np.ndarray]:
    """The definition of :func:`real_batch`'s images: :func:`mixup_np` on both outputs of :func:`pair_batch_np` -> (im_noisy, im_gt)."""
    im_noisy, im_gt = pair_batch_np(noisy_images, gt_images, params)
    return mixup_np(im_noisy, mix), mixup_np(im_gt, mix)


def hr_batch_np(images, params: BatchParams) -> np.ndarray:
    """The definition of :func:`hr_batch` (datasets/SISRDatasets.py:69-76): crop, ``/ 255`` as a true division, augmentation."""
    return _nchw([augment_np(u8_to_float_np(_crop_np(images, params, i), divide=True), params.flag[i]) for i in range(params.n)])


def philox4x32_np(counter: np.ndarray, key: np.ndarray, rounds: int = 10) -> np.ndarray:
    """Philox4x32 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ``counter`` uint32 [...,4], ``key`` uint32 [...,2]
    (broadcast against each other) -> uint32 [...,4]."""
    c = [np.asarray(counter)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(np.uint64) for k in range(2))
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def normal_words_np(per: int, seed: int, sample_ids, stream: int) -> np.ndarray:
    """uint32 [N, ceil(per/4), 4]: the generator's words, counter (e >> 2, stream, sample id low, high), key = the 64-bit seed."""
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1).view(np.uint64)
    nq = -(-int(per) // 4)
    counter = np.zeros((ids.shape[0], nq, 4), dtype=np.uint32)
    counter[..., 0] = np.arange(nq, dtype=np.uint32)
    counter[..., 1] = np.uint32(int(stream) & 0xFFFFFFFF)
    counter[..., 2] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    counter[..., 3] = (ids >> np.uint64(32)).astype(np.uint32)[:, None]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_np(counter, np.asarray([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))


def normal_np(shape, seed: int, sample_ids, stream: int = 0, dtype=np.float64) -> np.ndarray:
    """The definition of :func:`normal`: ``shape`` = (N, ...) -> standard normals of that shape, evaluated in ``dtype`` (float64: the
    definition; float32: the same formula at the device's precision).  Word pairs (w0, w1) and (w2, w3) each give two normals by Box-Muller
    with the exact 24-bit uniforms u1 = ((w >> 8) + 1) 2^-24, u2 = (w >> 8) 2^-24: r = sqrt(-2 log u1), (r cos 2 pi u2, r sin 2 pi u2);
    element e of a sample takes normal e & 3 of counter e >> 2."""
    shape = tuple(int(s) for s in shape)
    per = int(np.prod(shape[1:], dtype=np.int64))
    w = normal_words_np(per, seed, sample_ids, stream)
    if w.shape[0] != shape[0]:
        raise ValueError(f"{w.shape[0]} sample ids for a batch of {shape[0]}")
    dt = np.dtype(dtype).type
    u1 = ((w[..., 0::2] >> np.uint32(8)).astype(np.int64) + 1).astype(dt) * dt(2.0 ** -24)
    u2 = (w[..., 1::2] >> np.uint32(8)).astype(dt) * dt(2.0 ** -24)
    r = np.sqrt(dt(-2.0) * np.log(u1))
    ang = dt(2.0 * np.pi) * u2
    z = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=-1)          # [N, nq, pair, (cos, sin)]
    return np.ascontiguousarray(z.reshape(shape[0], -1)[:, :per]).reshape(shape).astype(dt)


def blur_kernels_np(lam1_sq, lam2_sq, theta, k_size: int = 21, sf: int = 2, shift: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The definition of :func:`blur_kernels`: ``sisr_eval.anisotropic_gaussian_kernel`` per sample -> (fp32 [N,1,k,k], fp32 [N,3])."""
    pairs = [sisr_eval.anisotropic_gaussian_kernel(k_size, sf, float(a), float(b), float(t), shift) for a, b, t in zip(lam1_sq, lam2_sq, theta)]
    return (np.stack([k for k, _ in pairs])[:, np.newaxis].astype(np.float32), np.stack([i for _, i in pairs]).astype(np.float32))


def sisr_batch_np(images, params: BatchParams, sf: int, k_size: int, noise: np.ndarray, downsampler: str = "bicubic", shift: bool = False):
    """The definition of :func:`sisr_batch`: ``noise`` fp32 [N,3,h,w] standard normals of the LR shape -> (im_hr, im_lr, im_blur, kinfo,
    nlevel) as numpy arrays (datasets/SISRDatasets.py:66-122)."""
    im_hr = hr_batch_np(images, params)
    kernel, kinfo = blur_kernels_np(params.lam1 ** 2, params.lam2 ** 2, params.theta, k_size, sf, shift)
    lrs, blurs = [], []
    for i in range(params.n):
        lr, blur = sisr_eval.synthesize_lr_np(np.ascontiguousarray(im_hr[i].transpose(1, 2, 0)), kernel[i, 0], sf,
                                              np.ascontiguousarray(np.asarray(noise[i], dtype=np.float32).transpose(1, 2, 0)),
                                              float(np.float32(params.std[i])), int(params.qf[i]), downsampler)
        lrs.append(lr)
        blurs.append(blur)
    return im_hr, _nchw(lrs), _nchw(blurs), kinfo, params.std.astype(np.float32).reshape(-1, 1, 1, 1)


# ---- the device entry points ----------------------------------------------------------------------------------------------------------------
def _check_call(pool, params, size: int, who: str, paired: bool = False) -> Tuple[int, int]:
    """Host-side checks of a batch call, before any device work -> (n, patch size)."""
    if not isinstance(pool, ImagePool):
        raise TypeError(f"{who}: pool must be an ImagePool, got {type(pool).__name__}")
    if paired and pool.data_b is None:
        raise ValueError(f"{who}: the pool has no second buffer; build it with ImagePool.paired")
    if not isinstance(params, (BatchParams, DeviceParams)):
        raise TypeError(f"{who}: params must be BatchParams or DeviceParams, got {type(params).__name__}")
    if params.shapes != pool.shapes:
        raise ValueError(f"{who}: the parameters were drawn for another pool")
    if isinstance(size, bool) or int(size) != size or int(size) != params.pch_size:
        raise ValueError(f"{who}: patch size {size!r} but the parameters were drawn for {params.pch_size}")
    return params.n, params.pch_size


def _on_device(pool: ImagePool, params, who: str, paired: bool = False, **tensors) -> DeviceParams:
    """Refuses CPU tensors, then uploads host parameters (one pinned, non-blocking copy)."""
    named = (("pool.data", pool.data), ("pool.table", pool.table)) + ((("pool.data_b", pool.data_b),) if paired else ())
    named += tuple((k, v) for k, v in tensors.items() if v is not None)
    if isinstance(params, DeviceParams):
        named += (("params", params.blob),)
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name} is on {t.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
        if t.device != pool.data.device:
            raise RuntimeError(f"{who}: the pool is on {pool.data.device}, {name} on {t.device}")
    return params.to(pool.data.device) if isinstance(params, BatchParams) else params


def _seed(seed) -> int:
    if isinstance(seed, (bool, Tensor)) or not isinstance(seed, int):
        raise TypeError(f"seed {seed!r}: a Python int is expected (it travels as a kernel argument)")
    return seed & 0xFFFFFFFFFFFFFFFF


def _ids(sample_ids, base_id: int, n: int, device: torch.device, who: str) -> Tensor:
    if sample_ids is None:
        return torch.arange(int(base_id), int(base_id) + n, dtype=torch.int64, device=device)
    if not isinstance(sample_ids, Tensor) or sample_ids.dtype != torch.int64 or tuple(sample_ids.shape) != (n,):
        raise ValueError(f"{who}: sample_ids must be an int64 tensor [{n}]")
    if not sample_ids.is_cuda:
        raise RuntimeError(f"{who}: sample_ids is on {sample_ids.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    if sample_ids.device != device:
        raise RuntimeError(f"{who}: sample_ids is on {sample_ids.device}, the batch on {device}")
    return sample_ids.contiguous()


def _patches(mode: int, pool: ImagePool, params: DeviceParams, noise, ids, seed: int, stream: int, clip: bool, outs) -> None:
    _native.check(_native.load().virnet_datagen_patches(mode, pool.data.data_ptr(), _native.ptr(pool.data_b), pool.table.data_ptr(), params.blob.data_ptr(),
                                                        params.n, params.pch_size, _native.ptr(noise), _native.ptr(ids), seed, stream, int(clip),
                                                        *[_native.ptr(o) for o in outs], _native.stream_handle()), "datagen_patches")


def denoise_batch(pool: ImagePool, params, pch_size: int, seed: int = 0, noise: Optional[Tensor] = None, sample_ids: Optional[Tensor] = None,
                  clip: bool = False, base_id: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """``SimulateTrain.__getitem__`` for a batch (datasets/DenoisingDatasets.py:217-253) -> (im_noisy [N,3,P,P], im_gt [N,3,P,P], sigma_map_gt
    [N,1,P,P]), fp32, one launch.  ``params``: :func:`draw_denoise_params`' result, or a :class:`DeviceParams` of it.  ``noise``: fp32
    [N,3,P,P] standard normals at source coordinates (before the augmentation) for exact parity with a host stream; None draws them in the
    kernel from ``seed`` and ``sample_ids`` (int64 [N] on the device, default ``base_id + arange(N)``), so a sample's noise depends on its id
    alone and ranks with disjoint ids draw disjoint streams.  ``clip`` clamps im_noisy to [0,1] (``SimulateTrain(clip=True)``)."""
    n, p = _check_call(pool, params, pch_size, "denoise_batch")
    if noise is not None:
        if not isinstance(noise, Tensor) or noise.dtype != torch.float32:
            raise TypeError("denoise_batch: noise must be a float32 tensor")
        if tuple(noise.shape) != (n, 3, p, p):
            raise ValueError(f"denoise_batch: noise must be {(n, 3, p, p)}, got {tuple(noise.shape)}")
    seed = _seed(seed)
    dp = _on_device(pool, params, "denoise_batch", noise=noise)
    dev = pool.data.device
    if noise is not None:
        noise = noise.contiguous()
    with torch.no_grad(), torch.cuda.device(dev):
        ids = None if noise is not None else _ids(sample_ids, base_id, n, dev, "denoise_batch")
        im_noisy = torch.empty((n, 3, p, p), dtype=torch.float32, device=dev)
        im_gt = torch.empty((n, 3, p, p), dtype=torch.float32, device=dev)
        sigma_map_gt = torch.empty((n, 1, p, p), dtype=torch.float32, device=dev)
        _patches(DENOISE, pool, dp, noise, ids, seed, STREAM_DENOISE, clip, (im_noisy, im_gt, sigma_map_gt))
    return im_noisy, im_gt, sigma_map_gt


def pair_batch(pool: ImagePool, params, pch_size: int) -> Tuple[Tensor, Tensor]:
    """``RealTrain`` / ``DataLMDB.__getitem__`` for a batch (datasets/DenoisingDatasets.py:74-99, 137-155) from a pool built with
    :meth:`ImagePool.paired` -> (im_noisy, im_gt), both [N,3,P,P] fp32 = ``u8 * fp32(1/255)``, cropped and augmented alike."""
    n, p = _check_call(pool, params, pch_size, "pair_batch", paired=True)
    dp = _on_device(pool, params, "pair_batch", paired=True)
    dev = pool.data.device
    with torch.no_grad(), torch.cuda.device(dev):
        im_noisy = torch.empty((n, 3, p, p), dtype=torch.float32, device=dev)
        im_gt = torch.empty((n, 3, p, p), dtype=torch.float32, device=dev)
        _patches(PAIR, pool, dp, None, None, 0, 0, False, (im_noisy, im_gt, None))
    return im_noisy, im_gt


def _check_mix(mix, n: int, who: str) -> None:
    if not isinstance(mix, (MixParams, DeviceMix)):
        raise TypeError(f"{who}: mix must be MixParams or DeviceMix, got {type(mix).__name__}")
    if mix.n != n:
        raise ValueError(f"{who}: the mix is of {mix.n} samples, the batch of {n}")


def _mix_on_device(mix, dev: torch.device, who: str) -> "DeviceMix":
    """Refuses a mix on another device, then uploads a host mix (one pinned, non-blocking copy)."""
    if isinstance(mix, DeviceMix):
        if mix.blob.device != dev:
            raise RuntimeError(f"{who}: the batch is on {dev}, mix on {mix.blob.device}")
        return mix
    return mix.to(dev)


def mixup(im_gt: Tensor, im_noisy: Tensor, mix) -> Tuple[Tensor, Tensor]:
    """``MixUp_AUG.aug(rgb_gt, rgb_noisy)`` (datasets/data_tools.py:19-30, train_denoising_real.py:163) with the draws of ``mix``
    (:func:`draw_mixup_params`, or a :class:`DeviceMix` of it) -> (im_gt, im_noisy), argument and result order as there: ``lam * x + (1 - lam)
    * x[perm]`` for both, fresh outputs, one launch (:func:`mixup_np` is the definition, met bit for bit).  Any two fp32 [N,C,H,W] tensors of
    one shape on one device: for batches that come from the caller's own loader; :func:`real_batch` mixes while it crops."""
    for name, t in (("im_gt", im_gt), ("im_noisy", im_noisy)):
        if not isinstance(t, Tensor) or t.dtype != torch.float32:
            raise TypeError(f"mixup: {name} must be a float32 tensor, got {t.dtype if isinstance(t, Tensor) else type(t).__name__}")
        if t.dim() != 4:
            raise ValueError(f"mixup: {name} must be [N,C,H,W], got {tuple(t.shape)}")
    if im_gt.shape != im_noisy.shape:
        raise ValueError(f"mixup: im_gt {tuple(im_gt.shape)} != im_noisy {tuple(im_noisy.shape)}")
    n, per = int(im_gt.shape[0]), int(np.prod(im_gt.shape[1:], dtype=np.int64))
    if not 1 <= n <= 65535 or not 1 <= per < 1 << 31:
        raise ValueError(f"mixup: shape {tuple(im_gt.shape)}: 1..65535 samples of 1..2^31-1 elements")
    _check_mix(mix, n, "mixup")
    for name, t in (("im_gt", im_gt), ("im_noisy", im_noisy)):
        if not t.is_cuda:
            raise RuntimeError(f"mixup: {name} is on {t.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    dev = im_gt.device
    if im_noisy.device != dev:
        raise RuntimeError(f"mixup: im_gt is on {dev}, im_noisy on {im_noisy.device}")
    dm = _mix_on_device(mix, dev, "mixup")
    with torch.no_grad(), torch.cuda.device(dev):
        a, b = im_gt.detach().contiguous(), im_noisy.detach().contiguous()
        out_a = torch.empty(tuple(a.shape), dtype=torch.float32, device=dev)
        out_b = torch.empty(tuple(a.shape), dtype=torch.float32, device=dev)
        _native.check(_native.load().virnet_mixup(a.data_ptr(), b.data_ptr(), dm.blob.data_ptr(), out_a.data_ptr(), out_b.data_ptr(), n, per,
                                                  _native.stream_handle()), "mixup")
    return out_a, out_b


def real_batch(pool: ImagePool, params, pch_size: int, mix, k_size: Optional[int] = 7, floor: float = 1e-10):
    """The batch of the real-noise training step (train_denoising_real.py:160-164) from a pool built with :meth:`ImagePool.paired` ->
    (im_noisy, im_gt, sigma_gt), all [N,3,P,P] fp32, output order as :func:`pair_batch`: the paired patches (``params``:
    :func:`draw_pair_params`' result or a :class:`DeviceParams` of it), mixed by ``mix`` (:func:`draw_mixup_params`' result or a
    :class:`DeviceMix` of it) while they are cropped -- one launch, :func:`real_batch_np` is its definition, met bit for bit -- and
    ``sigma_gt = max(G_k (*) (im_noisy - im_gt)**2, floor)`` by ``elbo.noise_estimate`` on the two in a second launch (``k_size``: the
    reference's ``var_window``).  ``k_size=None`` skips that launch and returns None for ``sigma_gt``.  Each rank mixes within its own
    batch, as the reference does."""
    from . import elbo
    n, p = _check_call(pool, params, pch_size, "real_batch", paired=True)
    _check_mix(mix, n, "real_batch")
    if k_size is not None:
        if isinstance(k_size, bool) or int(k_size) != k_size or int(k_size) % 2 == 0 or not 1 <= int(k_size) <= elbo.MAX_WINDOW:
            raise ValueError(f"real_batch: window size {k_size!r}: odd sizes 1..{elbo.MAX_WINDOW} are supported")
        if int(k_size) // 2 >= p:
            raise ValueError(f"real_batch: padding {int(k_size) // 2} of a {k_size}x{k_size} window must be smaller than the {p}x{p} patch")
        if 3 * n > 65535 or p > 32768:
            raise ValueError(f"real_batch: {n} samples of {p}x{p}: the variance prior takes at most 21845 samples of at most 32768x32768")
    dp = _on_device(pool, params, "real_batch", paired=True, mix=mix.blob if isinstance(mix, DeviceMix) else None)
    dev = pool.data.device
    dm = _mix_on_device(mix, dev, "real_batch")
    with torch.no_grad(), torch.cuda.device(dev):
        im_noisy = torch.empty((n, 3, p, p), dtype=torch.float32, device=dev)
        im_gt = torch.empty((n, 3, p, p), dtype=torch.float32, device=dev)
        _native.check(_native.load().virnet_datagen_pair_mix(pool.data.data_ptr(), pool.data_b.data_ptr(), pool.table.data_ptr(), dp.blob.data_ptr(),
                                                             dm.blob.data_ptr(), n, p, im_noisy.data_ptr(), im_gt.data_ptr(),
                                                             _native.stream_handle()), "datagen_pair_mix")
    sigma_gt = None if k_size is None else elbo.noise_estimate(im_noisy, im_gt, int(k_size), floor)
    return im_noisy, im_gt, sigma_gt


def hr_batch(pool: ImagePool, params, hr_size: int) -> Tensor:
    """The HR patches of ``GeneralTrainFloder.__getitem__`` (datasets/SISRDatasets.py:69-76) -> [N,3,P,P] fp32 = ``u8 / 255`` as a true
    division, cropped and augmented."""
    n, p = _check_call(pool, params, hr_size, "hr_batch")
    dp = _on_device(pool, params, "hr_batch")
    dev = pool.data.device
    with torch.no_grad(), torch.cuda.device(dev):
        im_hr = torch.empty((n, 3, p, p), dtype=torch.float32, device=dev)
        _patches(HR, pool, dp, None, None, 0, 0, False, (im_hr, None, None))
    return im_hr


def normal(shape, seed: int, sample_ids: Optional[Tensor] = None, stream: int = 0, device=None, base_id: int = 0) -> Tensor:
    """Standard normals of ``shape`` = (N, ...) as fp32 on the device, by the generator :func:`denoise_batch` draws from (:func:`normal_np`
    is its definition): sample n's values depend on ``seed``, ``stream`` and ``sample_ids[n]`` alone."""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 1 or any(s < 1 for s in shape):
        raise ValueError(f"normal: shape {shape}: at least one dimension, all positive")
    n, per = shape[0], int(np.prod(shape[1:], dtype=np.int64))
    if n > 65535 or per >= 1 << 31:
        raise ValueError(f"normal: shape {shape}: at most 65535 samples of fewer than 2^31 elements")
    seed = _seed(seed)
    if sample_ids is not None and isinstance(sample_ids, Tensor) and device is None:
        device = sample_ids.device
    dev = _require_device("cuda" if device is None else device, "normal")
    with torch.no_grad(), torch.cuda.device(dev):
        ids = _ids(sample_ids, base_id, n, dev, "normal")
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        _native.check(_native.load().virnet_datagen_normal(out.data_ptr(), n, per, ids.data_ptr(), seed, int(stream), _native.stream_handle()),
                      "datagen_normal")
    return out


def blur_kernels(lam1_sq: Tensor, lam2_sq: Tensor, theta: Tensor, k_size: int = 21, sf: int = 2, shift: bool = False) -> Tuple[Tensor, Tensor]:
    """``util_sisr.shifted_anisotropic_Gaussian`` per sample (utils/util_sisr.py:60-93; host definition ``sisr_eval.anisotropic_gaussian_kernel``):
    fp64 [N] device tensors of the two eigenvalues of the covariance and its angle -> (kernel [N,1,k,k] fp32, kinfo [N,3] fp32 = var_x,
    var_y, rho), computed in fp64.  k odd and <= 25, the range ``degrade`` takes."""
    for name, t in (("lam1_sq", lam1_sq), ("lam2_sq", lam2_sq), ("theta", theta)):
        if not isinstance(t, Tensor) or t.dtype != torch.float64 or t.dim() != 1:
            raise TypeError(f"blur_kernels: {name} must be a 1-D float64 tensor")
    n, dev = int(lam1_sq.shape[0]), lam1_sq.device
    if n < 1 or lam2_sq.shape[0] != n or theta.shape[0] != n:
        raise ValueError("blur_kernels: lam1_sq, lam2_sq and theta must be [N], N >= 1")
    if isinstance(k_size, bool) or int(k_size) != k_size or int(k_size) % 2 == 0 or not 1 <= int(k_size) <= MAX_KERNEL:
        raise ValueError(f"kernel size {k_size!r}: odd sizes 1..{MAX_KERNEL} are supported")
    if isinstance(sf, bool) or int(sf) != sf or not 1 <= int(sf) <= degrade.MAX_SF:
        raise ValueError(f"sf {sf!r}: integer scale factors 1..{degrade.MAX_SF} are supported")
    k = int(k_size)
    for name, t in (("lam1_sq", lam1_sq), ("lam2_sq", lam2_sq), ("theta", theta)):
        if not t.is_cuda:
            raise RuntimeError(f"blur_kernels: {name} is on {t.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
        if t.device != dev:
            raise RuntimeError(f"blur_kernels: lam1_sq is on {dev}, {name} on {t.device}")
    with torch.no_grad(), torch.cuda.device(dev):
        a, b, t = lam1_sq.contiguous(), lam2_sq.contiguous(), theta.contiguous()
        kernel = torch.empty((n, 1, k, k), dtype=torch.float32, device=dev)
        kinfo = torch.empty((n, 3), dtype=torch.float32, device=dev)
        _native.check(_native.load().virnet_datagen_blur_kernels(a.data_ptr(), b.data_ptr(), t.data_ptr(), n, k, int(sf), int(bool(shift)),
                                                                 kernel.data_ptr(), kinfo.data_ptr(), _native.stream_handle()), "datagen_blur_kernels")
    return kernel, kinfo


def sisr_batch(pool: ImagePool, params, hr_size: int, sf: int, k_size: int = 21, seed: int = 0, downsampler: str = "bicubic", shift: bool = False,
               noise: Optional[Tensor] = None, sample_ids: Optional[Tensor] = None, base_id: int = 0):
    """``GeneralTrainFloder.__getitem__`` collated (datasets/SISRDatasets.py:66-122) -> (im_hr [N,3,P,P], im_lr, im_blur [N,3,P/sf,P/sf],
    kinfo [N,3], nlevel [N,1,1,1]), fp32: :func:`hr_batch`, :func:`blur_kernels`, :func:`normal` with stream 1 at the LR shape (or the
    caller's ``noise``) and ``degrade.synthesize_lr``; samples whose ``qf`` is not 0 end in the JPEG round trip (skipped altogether when the
    parameters last uploaded held no such sample)."""
    n, p = _check_call(pool, params, hr_size, "sisr_batch")
    if isinstance(sf, bool) or int(sf) != sf or not 1 <= int(sf) <= degrade.MAX_SF:
        raise ValueError(f"sf {sf!r}: integer scale factors 1..{degrade.MAX_SF} are supported")
    sf = int(sf)
    lr_shape = (n, 3, -(-p // sf), -(-p // sf))
    if noise is not None and (not isinstance(noise, Tensor) or noise.dtype != torch.float32 or tuple(noise.shape) != lr_shape):
        raise ValueError(f"sisr_batch: noise must be a float32 tensor of the LR shape {lr_shape}")
    dp = _on_device(pool, params, "sisr_batch", noise=noise)
    im_hr = hr_batch(pool, dp, p)
    kernel, kinfo = blur_kernels(dp.lam1_sq, dp.lam2_sq, dp.theta, k_size, sf, shift)
    if noise is None:
        noise = normal(lr_shape, seed, sample_ids, STREAM_SISR_LR, pool.data.device, base_id)
    std = dp.std
    im_lr, im_blur = degrade.synthesize_lr(im_hr, kernel, sf, noise, std, dp.qf if dp.any_qf else None, downsampler)
    return im_hr, im_lr, im_blur, kinfo, std.reshape(n, 1, 1, 1)


# ---- the validation set (SimulateTest) ------------------------------------------------------------------------------------------------------
def nearest_exact_indices(size: int, src: int = SIMTEST_MAP) -> np.ndarray:
    """int32 [size]: the source index of every destination index of ``cv2.resize(..., INTER_NEAREST_EXACT)`` from ``src`` to ``size`` samples,
    ``floor((dst + 0.5) * src / size)`` evaluated in fp64 by ``eval.resize_nearest_exact``'s own expression (the device only gathers)."""
    if isinstance(size, bool) or int(size) != size or int(size) < 1:
        raise ValueError(f"size {size!r}: a positive integer is expected")
    size, src = int(size), int(src)
    return np.minimum(np.floor((np.arange(size) + 0.5) * (src / size)).astype(np.int64), src - 1).astype(np.int32)


def simulate_sigma_map() -> np.ndarray:
    """``SimulateTest.generate_sigma_map`` (datasets/DenoisingDatasets.py:278-284): the 256 x 256 peaks surface rescaled to [10/255, 75/255]
    in fp64, then rounded to fp32."""
    k = veval.peaks(SIMTEST_MAP)
    down, up = 10 / 255., 75 / 255.
    return (down + (k - k.min()) / (k.max() - k.min()) * (up - down)).astype(np.float32)


def simulate_noise(shapes, seed: int = 1000) -> np.ndarray:
    """``SimulateTest.generate_noise`` (:266-276): ONE fp32 array [h_max, w_max, 3] for the whole set, from ``default_rng(seed)``."""
    h_max = max([1] + [int(h) for h, _ in shapes])
    w_max = max([1] + [int(w) for _, w in shapes])
    return np.random.default_rng(seed=seed).standard_normal(size=[h_max, w_max, 3], dtype=np.float32)


def simulate_test_np(images, indices, noise: np.ndarray, sigma_map: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The definition of :meth:`SimulateTestSet.batch`: ``SimulateTest.__getitem__`` (:286-296) for the images ``indices`` of one common
    shape -> (im_noisy, im_gt), fp32 [n,3,h,w].  ``im_gt = u8 / 255`` as a true fp32 division (``util_image.imread``,
    utils/util_image.py:206 -- not the ``u8 * fp32(1/255)`` of the training set, which differs in the last bit for 126 byte values);
    ``sigma = resize_nearest_exact(sigma_map, h, w)``; ``im_noisy = im_gt + noise[:h, :w] * sigma[:, :, None]``, product and sum each
    rounded to fp32."""
    noisy, gts = [], []
    for i in indices:
        im_gt = u8_to_float_np(images[int(i)], divide=True)
        h, w = im_gt.shape[:2]
        sigma = veval.resize_nearest_exact(np.asarray(sigma_map, dtype=np.float32), h, w)
        noisy.append(im_gt + np.asarray(noise, dtype=np.float32)[:h, :w] * sigma[:, :, np.newaxis])
        gts.append(im_gt)
    if len({g.shape for g in gts}) > 1:
        raise ValueError(f"simulate_test_np: the images {list(indices)} are not of one shape")
    return _nchw(noisy), _nchw(gts)


@functools.lru_cache(maxsize=256)
def _device_nearest(size: int, device: str) -> Tensor:
    """:func:`nearest_exact_indices` on the device, built once per (size, device): no per-call host-to-device copy."""
    with _native.capture_lock:
        return torch.from_numpy(nearest_exact_indices(size)).to(torch.device(device))


class SimulateTestSet:
    """``SimulateTest(im_list, seed)`` (datasets/DenoisingDatasets.py:255-296) over the images of an :class:`ImagePool`, on the pool's device:
    the uint8 pool, the single noise array ``rng.standard_normal([h_max, w_max, 3], dtype=float32)`` -- drawn on the host once, uploaded once
    -- and the 256 x 256 fp32 sigma map (``noise``, ``sigma_map``: device tensors; ``noise_np``, ``sigma_map_np``: the host arrays).
    :meth:`batch` is one launch and does not synchronise; :func:`simulate_test_np` is its definition, met bit for bit.  A set may be built
    over a CPU pool (for the definition); :meth:`batch` refuses it."""

    def __init__(self, pool: ImagePool, seed: int = 1000):
        if not isinstance(pool, ImagePool):
            raise TypeError(f"SimulateTestSet: pool must be an ImagePool, got {type(pool).__name__}")
        if isinstance(seed, (bool, Tensor)) or not isinstance(seed, int) or seed < 0:
            raise TypeError(f"SimulateTestSet: seed {seed!r}: a non-negative Python int is expected")
        self.pool, self.seed = pool, seed
        self.noise_np = simulate_noise(pool.shapes, seed)
        self.sigma_map_np = simulate_sigma_map()
        self.h_max, self.w_max = int(self.noise_np.shape[0]), int(self.noise_np.shape[1])
        with _native.capture_lock:
            self.noise: Tensor = torch.from_numpy(self.noise_np).to(pool.device)
            self.sigma_map: Tensor = torch.from_numpy(self.sigma_map_np).to(pool.device)
        self._indices: dict = {}

    def __len__(self) -> int:
        return len(self.pool)

    def groups(self) -> List[List[int]]:
        """The image indices grouped by shape, groups in order of their first image: one :meth:`batch` call each."""
        by_shape: dict = {}
        for i, s in enumerate(self.pool.shapes):
            by_shape.setdefault(s, []).append(i)
        return list(by_shape.values())

    def _check_indices(self, indices) -> Tuple[List[int], int, int]:
        if isinstance(indices, Tensor):
            raise TypeError("SimulateTestSet.batch: indices must be host integers (they select the images whose common shape sizes the launch)")
        idx = [indices] if isinstance(indices, (int, np.integer)) and not isinstance(indices, bool) else list(indices)
        if not idx or len(idx) > 65535:
            raise ValueError(f"SimulateTestSet.batch: indices: {len(idx)} images (1..65535 expected)")
        for k, i in enumerate(idx):
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)):
                raise TypeError(f"SimulateTestSet.batch: indices[{k}] = {i!r}: an integer is expected")
            if not 0 <= int(i) < len(self.pool):
                raise ValueError(f"SimulateTestSet.batch: indices[{k}] = {i} outside 0..{len(self.pool) - 1}")
        idx = [int(i) for i in idx]
        h, w = self.pool.shapes[idx[0]]
        for k, i in enumerate(idx):
            if self.pool.shapes[i] != (h, w):
                raise ValueError(f"SimulateTestSet.batch: indices[{k}] = {i} names a {self.pool.shapes[i][0]}x{self.pool.shapes[i][1]} image, "
                                 f"indices[0] a {h}x{w} one: a batch holds images of one shape (see groups())")
        if 3 * h * w >= 1 << 31:
            raise ValueError(f"SimulateTestSet.batch: images of {h}x{w}: fewer than 2^31 / 3 pixels are expected")
        return idx, h, w

    def batch(self, indices) -> Tuple[Tensor, Tensor]:
        """``SimulateTest.__getitem__`` for the pool images ``indices`` (host integers, one common shape, repeats allowed) -> (im_noisy,
        im_gt), fp32 [n,3,h,w], in one launch on the current stream."""
        idx, h, w = self._check_indices(indices)
        pool = self.pool
        for name, t in (("pool.data", pool.data), ("pool.table", pool.table), ("noise", self.noise), ("sigma_map", self.sigma_map)):
            if not t.is_cuda:
                raise RuntimeError(f"SimulateTestSet.batch: {name} is on {t.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
            if t.device != pool.data.device:
                raise RuntimeError(f"SimulateTestSet.batch: the pool is on {pool.data.device}, {name} on {t.device}")
        dev = pool.data.device
        n = len(idx)
        with torch.no_grad(), torch.cuda.device(dev):
            d_idx = self._indices.get(tuple(idx))
            if d_idx is None:
                with _native.capture_lock:      # (pinned allocation is not permitted while any stream of the process captures)
                    staged = torch.empty(n, dtype=torch.int32, pin_memory=True)
                staged.numpy()[:] = np.asarray(idx, dtype=np.int32)
                d_idx = torch.empty(n, dtype=torch.int32, device=dev)
                d_idx.copy_(staged, non_blocking=True)
                if len(self._indices) < 1024:
                    self._indices[tuple(idx)] = d_idx
            ys, xs = _device_nearest(h, str(dev)), _device_nearest(w, str(dev))
            im_noisy = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
            im_gt = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
            _native.check(_native.load().virnet_datagen_simulate_test(pool.data.data_ptr(), pool.table.data_ptr(), d_idx.data_ptr(), self.noise.data_ptr(),
                                                                      self.sigma_map.data_ptr(), ys.data_ptr(), xs.data_ptr(), n, h, w, self.h_max,
                                                                      self.w_max, im_noisy.data_ptr(), im_gt.data_ptr(), _native.stream_handle()),
                          "datagen_simulate_test")
        return im_noisy, im_gt


# ---- the validation set of the SISR training (GeneralTest) ----------------------------------------------------------------------------------
GENERAL_LAMBDA = 1.6 ** 2          # datasets/SISRDatasets.py:174-175: the fixed isotropic kernel of the validation set
GENERAL_NLEVEL = 2.55 / 255        # :194: the fixed noise level (a Python double; it meets the float32 noise array as a float32)
GENERAL_QF = 40                    # :199


def general_noise(shapes, sf: int, seed: int = 10000) -> np.ndarray:
    """``GeneralTest.generate_noise`` (datasets/SISRDatasets.py:151-163): ONE fp32 array [ceil(h_max/sf), ceil(w_max/sf), 3] for the whole
    set, ``torch.randn`` from a CPU generator seeded with ``seed`` (``h_max``, ``w_max`` over the images as they are read, before the
    mod-crop)."""
    h_max = max([1] + [int(h) for h, _ in shapes])
    w_max = max([1] + [int(w) for _, w in shapes])
    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.randn([math.ceil(h_max / sf), math.ceil(w_max / sf), 3], generator=g, dtype=torch.float32).numpy()


def _check_general(sf, k_size, downsampler, noise_type) -> Tuple[int, int, str, str]:
    if isinstance(sf, bool) or int(sf) != sf or not 1 <= int(sf) <= degrade.MAX_SF:
        raise ValueError(f"sf {sf!r}: integer scale factors 1..{degrade.MAX_SF} are supported")
    if isinstance(k_size, bool) or int(k_size) != k_size or int(k_size) % 2 == 0 or not 1 <= int(k_size) <= MAX_KERNEL:
        raise ValueError(f"kernel size {k_size!r}: odd sizes 1..{MAX_KERNEL} are supported")
    mode = str(downsampler).lower()
    if mode not in ("direct", "bicubic"):
        raise ValueError("downsampler must be 'direct' or 'bicubic'")
    if noise_type not in ("Gaussian", "JPEG"):
        raise ValueError(f"noise_type {noise_type!r}: 'Gaussian' or 'JPEG' is expected")
    return int(sf), int(k_size), mode, noise_type


def general_test_np(images, sf: int, k_size: int = 21, kernel_shift: bool = False, downsampler: str = "bicubic", noise_type: str = "Gaussian",
                    noise: Optional[np.ndarray] = None, seed: int = 10000) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """The definition of :class:`GeneralTestSet`: ``GeneralTest.__getitem__`` (datasets/SISRDatasets.py:165-207) per uint8 [H,W,3] image ->
    [(im_hr fp32 [3,H',W'], im_lr fp32 [3,h,w], kinfo fp32 [3])].  ``noise``: the set's array (default :func:`general_noise` of the images'
    shapes).  The dtypes are the reference's: ``u8 / 255`` as a true fp32 division, the blur in fp32; "direct" stays fp32 throughout,
    while the bicubic result stays float64 until it has met the noise and is cast afterwards; the JPEG branch casts to fp32 before the
    round trip."""
    sf, k_size, mode, noise_type = _check_general(sf, k_size, downsampler, noise_type)
    images = _check_images(images, "general_test_np")
    if noise is None:
        noise = general_noise([im.shape[:2] for im in images], sf, seed)
    noise = np.asarray(noise, dtype=np.float32)
    kernel, kinfo = sisr_eval.anisotropic_gaussian_kernel(k_size, sf, GENERAL_LAMBDA, GENERAL_LAMBDA, 0.0, bool(kernel_shift))
    out = []
    for u8 in images:
        im_hr = sisr_eval.modcrop(u8_to_float_np(u8, divide=True), sf)
        blur = np.clip(sisr_eval.ndimage.convolve(im_hr, kernel[:, :, np.newaxis], mode="reflect"), 0.0, 1.0)
        im_blur = blur[::sf, ::sf] if mode == "direct" else sisr_eval.bicubic_downscale(blur, sf)
        h, w = im_blur.shape[:2]
        if noise.shape[0] < h or noise.shape[1] < w:
            raise ValueError(f"general_test_np: the noise array {noise.shape} is smaller than an LR image {h}x{w}")
        im_lr = np.clip(im_blur + noise[:h, :w] * np.float32(GENERAL_NLEVEL), 0.0, 1.0).astype(np.float32)
        if noise_type == "JPEG":
            im_lr = veval.jpeg_compress(im_lr, GENERAL_QF)
        out.append((np.ascontiguousarray(im_hr.transpose(2, 0, 1)), np.ascontiguousarray(im_lr.transpose(2, 0, 1)).astype(np.float32),
                    kinfo.astype(np.float32)))
    return out


class GeneralTestSet:
    """``GeneralTest(hr_dir, sf, k_size, kernel_shift, downsampler, seed, noise_type)`` (datasets/SISRDatasets.py:124-207) over the images
    of an :class:`ImagePool` on a ROCm device.  The set does not change between epochs, so every image's ``(im_hr, im_lr, kinfo)`` is built
    ONCE here with the device operators (``degrade.synthesize_lr`` on the mod-cropped ``u8 / 255`` image, the fixed isotropic 1.6 kernel,
    the crop ``noise[:h, :w]`` of the single :func:`general_noise` array and the constant level ``fp32(2.55/255)``; ``"JPEG"`` ends in the
    quality-40 round trip) and stays resident, stacked per shape.  :meth:`batch` then only hands out views.  :func:`general_test_np` is the
    definition.

    Device memory: the set holds every HR and LR image in fp32 for its lifetime (15 bytes per HR pixel at sf 2).  A selection that is not
    a run of neighbours within one group (the validation stage asks for none) is gathered into NEW tensors, and the set keeps up to
    ``GATHER_CACHE`` of those, so that repeating it launches nothing; selections beyond that are gathered on every call."""

    GATHER_CACHE = 16

    def __init__(self, pool: ImagePool, sf: int, k_size: int = 21, kernel_shift: bool = False, downsampler: str = "bicubic",
                 noise_type: str = "Gaussian", seed: int = 10000):
        if not isinstance(pool, ImagePool):
            raise TypeError(f"GeneralTestSet: pool must be an ImagePool, got {type(pool).__name__}")
        if isinstance(seed, (bool, Tensor)) or not isinstance(seed, int) or seed < 0:
            raise TypeError(f"GeneralTestSet: seed {seed!r}: a non-negative Python int is expected")
        self.sf, self.k_size, self.downsampler, self.noise_type = _check_general(sf, k_size, downsampler, noise_type)
        self.kernel_shift, self.seed, self.pool = bool(kernel_shift), seed, pool
        dev = _require_device(pool.device, "GeneralTestSet")
        sf = self.sf
        self.shapes: List[Tuple[int, int]] = [(h - h % sf, w - w % sf) for h, w in pool.shapes]
        for i, (h, w) in enumerate(self.shapes):
            if self.k_size // 2 >= min(h, w):
                raise ValueError(f"GeneralTestSet: image {i} is {h}x{w} after the mod-crop, too small for a {self.k_size}x{self.k_size} kernel")
        self.noise_np = general_noise(pool.shapes, sf, seed)
        kernel, kinfo = sisr_eval.anisotropic_gaussian_kernel(self.k_size, sf, GENERAL_LAMBDA, GENERAL_LAMBDA, 0.0, self.kernel_shift)
        by_shape: dict = {}
        for i, s in enumerate(self.shapes):
            by_shape.setdefault(s, []).append(i)
        self._groups: List[List[int]] = list(by_shape.values())
        self._where = {i: (g, k) for g, group in enumerate(self._groups) for k, i in enumerate(group)}
        self._cache: dict = {}
        self._gathered = 0
        offsets = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in pool.shapes])]).astype(np.int64)
        with _native.capture_lock, torch.no_grad(), torch.cuda.device(dev):
            self.noise: Tensor = torch.from_numpy(self.noise_np).to(dev)
            lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(dev)      # u8 / 255 as a true division
            d_kernel = torch.from_numpy(kernel.astype(np.float32)[np.newaxis, np.newaxis]).to(dev)
            d_kinfo = torch.from_numpy(kinfo.astype(np.float32)).to(dev)
            std = torch.from_numpy(np.asarray([GENERAL_NLEVEL], dtype=np.float32)).to(dev)
            qf = torch.from_numpy(np.asarray([GENERAL_QF], dtype=np.int32)).to(dev) if self.noise_type == "JPEG" else None
            self._stacks = []
            for group in self._groups:
                hrs, lrs = [], []
                for i in group:
                    (h0, w0), (h, w) = pool.shapes[i], self.shapes[i]
                    u8 = pool.data[int(offsets[i]):int(offsets[i + 1])].view(h0, w0, 3)[:h, :w]
                    im_hr = lut[u8.long()].permute(2, 0, 1).contiguous().unsqueeze(0)
                    hl, wl = -(-h // sf), -(-w // sf)
                    crop = self.noise[:hl, :wl].permute(2, 0, 1).contiguous().unsqueeze(0)
                    im_lr, _ = degrade.synthesize_lr(im_hr, d_kernel, sf, crop, std, qf, self.downsampler)
                    hrs.append(im_hr)
                    lrs.append(im_lr)
                self._stacks.append((torch.cat(hrs), torch.cat(lrs), d_kinfo.unsqueeze(0).repeat(len(group), 1)))

    def __len__(self) -> int:
        return len(self.shapes)

    def groups(self) -> List[List[int]]:
        """The image indices grouped by (mod-cropped) shape, groups in order of their first image."""
        return [list(g) for g in self._groups]

    def batch(self, indices) -> Tuple[Tensor, Tensor, Tensor]:
        """``GeneralTest.__getitem__`` collated for the images ``indices`` (host integers, one common shape) -> (im_hr [n,3,H,W], im_lr
        [n,3,h,w], kinfo [n,3]), fp32.  A run of neighbours of one :meth:`groups` entry is a view of the resident stack; any other
        selection is gathered and (the first ``GATHER_CACHE`` of them) kept: the second call with the same indices launches nothing."""
        if isinstance(indices, Tensor):
            raise TypeError("GeneralTestSet.batch: indices must be host integers")
        idx = [indices] if isinstance(indices, (int, np.integer)) and not isinstance(indices, bool) else list(indices)
        if not idx:
            raise ValueError("GeneralTestSet.batch: no indices")
        for k, i in enumerate(idx):
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)):
                raise TypeError(f"GeneralTestSet.batch: indices[{k}] = {i!r}: an integer is expected")
            if not 0 <= int(i) < len(self):
                raise ValueError(f"GeneralTestSet.batch: indices[{k}] = {i} outside 0..{len(self) - 1}")
        idx = tuple(int(i) for i in idx)
        hit = self._cache.get(idx)
        if hit is not None:
            return hit
        g, k0 = self._where[idx[0]]
        for k, i in enumerate(idx):
            if self._where[i][0] != g:
                raise ValueError(f"GeneralTestSet.batch: indices[{k}] = {i} names a {self.shapes[i][0]}x{self.shapes[i][1]} image, indices[0] a "
                                 f"{self.shapes[idx[0]][0]}x{self.shapes[idx[0]][1]} one: a batch holds images of one shape (see groups())")
        pos = [self._where[i][1] for i in idx]
        stack = self._stacks[g]
        if pos == list(range(k0, k0 + len(pos))):
            out = tuple(t[k0:k0 + len(pos)] for t in stack)
            self._cache[idx] = out          # (views: no memory of their own)
        else:
            with _native.capture_lock, torch.cuda.device(stack[0].device):
                sel = torch.tensor(pos, dtype=torch.int64).to(stack[0].device)
                out = tuple(t.index_select(0, sel) for t in stack)
            if self._gathered < self.GATHER_CACHE:
                self._gathered += 1
                self._cache[idx] = out
        return out
