"""LPIPS v0.1 with the AlexNet backbone (``lpips.LPIPS(net='alex')``, ``spatial=False``, eval mode) for the SISR table's third column
(the reference: scripts/sisr_virnet_syn.py:96,158-161,169), from weights the caller supplies: neither the ``lpips`` package nor
``torchvision`` is imported.  INTEGRATION.md says how to export the pretrained weights where the package is installed.

The definition, for a uint8 RGB image ``u`` [3,H,W]:

  1. ``x = (u - 127.5) / 127.5`` (util_image.normalize_lpips, utils/util_image.py:118-126);
  2. the scaling layer ``x = (x - shift) / scale`` per channel;
  3. five taps, each after its ReLU: conv 3->64 11x11 /4 pad 2; max-pool 3x3 /2, conv 64->192 5x5 pad 2; max-pool 3x3 /2, conv 192->384
     3x3 pad 1; conv 384->256 3x3 pad 1; conv 256->256 3x3 pad 1 -- all with bias and ZERO padding of the scaled input;
  4. per tap ``n(f) = f / (sqrt(sum_c f_c^2) + 1e-10)`` and ``d_l = mean_hw sum_c w_lc (n(f0)_c - n(f1)_c)^2``;
  5. ``LPIPS = d_1 + ... + d_5``.

:func:`distance_torch` / :func:`features_torch` are that definition in plain torch ops on any device (the host form, and in float64 the
tests' yardstick); :func:`distance` / :func:`features` run csrc/lpips.hip: fp32 features (every value one k-ordered fmaf chain), fp64
scoring, nine launches, no atomics, no host synchronisation.  Device results are bitwise reproducible, do not depend on the batch a pair
sits in or on which of the two images comes first, and identical images give exactly 0.0.  Not differentiable.

Both pools need three rows, so the smallest image is 31 x 31.
"""
from __future__ import annotations

import ctypes as C
import zlib
from typing import Dict, List, Mapping, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from . import _native

MIN_SIZE = 31
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (cout, cin, kernel, stride, pad) of conv1..5; a 3x3 / stride 2 max-pool precedes conv2 and conv3
CONVS = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))
CHANNELS = tuple(c[0] for c in CONVS)
_SLICES = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")     # layout (A): torchvision's feature indices


class LpipsWeights:
    """The fp32 CPU originals -- ``conv_w[i]`` [cout,cin,k,k], ``conv_b[i]`` [cout], ``lin[i]`` [cout], ``shift`` / ``scale`` [3] -- and, per
    device, the packed copies the kernels read (made on first use; :meth:`prepare` makes them ahead of a graph capture).  A plain object
    that holds tensors only: ``copy.deepcopy`` and ``torch.save`` work and drop the device copies."""

    def __init__(self, conv_w, conv_b, lin, shift=None, scale=None):
        def f32(t, shape, what):
            t = torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous().clone()
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{what} has shape {tuple(t.shape)}, {tuple(shape)} expected")
            return t
        if len(conv_w) != 5 or len(conv_b) != 5 or len(lin) != 5:
            raise ValueError("LpipsWeights needs five convolution weights, five biases and five lin vectors")
        self.conv_w = [f32(t, (co, ci, k, k), f"conv{i + 1}.weight") for i, (t, (co, ci, k, _, _)) in enumerate(zip(conv_w, CONVS))]
        self.conv_b = [f32(t, (co,), f"conv{i + 1}.bias") for i, (t, (co, *_)) in enumerate(zip(conv_b, CONVS))]
        self.lin = [f32(t, (co,), f"lin{i + 1}") for i, (t, (co, *_)) in enumerate(zip(lin, CONVS))]
        self.shift = f32(SHIFT if shift is None else shift, (3,), "shift")
        self.scale = f32(SCALE if scale is None else scale, (3,), "scale")
        self._packed: Dict[torch.device, dict] = {}

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_packed"] = {}
        return state

    def tensors(self) -> Dict[str, Tensor]:
        """The flat layout (B) :func:`load_weights` reads back."""
        out = {}
        for i in range(5):
            out[f"conv{i + 1}.weight"], out[f"conv{i + 1}.bias"], out[f"lin{i + 1}"] = self.conv_w[i], self.conv_b[i], self.lin[i]
        out["shift"], out["scale"] = self.shift, self.scale
        return out

    def prepare(self, device) -> dict:
        """The packed device copies for ``device``: conv1 as [363][64] with k = (c, ky, kx), conv2..5 as [k*k*cin][cout] with
        k = (ky, kx, c) (include/virnet_hip.h: virnet_lpips_weights)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"weights asked for {device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._packed.get(device)
        if hit is not None:
            return hit

        def up(t):
            d = torch.empty(t.shape, dtype=torch.float32, device=device)
            d.copy_(t)
            return d
        packed = [self.conv_w[0].reshape(64, -1).t().contiguous()]
        packed += [w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous() for w in self.conv_w[1:]]
        hit = {"conv_w": [up(t) for t in packed], "conv_b": [up(t) for t in self.conv_b], "lin": [up(t) for t in self.lin]}
        self._packed[device] = hit
        return hit

    def drop_device_copies(self) -> None:
        self._packed = {}

    def _desc(self, device) -> "_native.LpipsWeightsDesc":
        p = self.prepare(device)
        d = _native.LpipsWeightsDesc()
        for i in range(5):
            d.conv_w[i], d.conv_b[i], d.lin[i] = p["conv_w"][i].data_ptr(), p["conv_b"][i].data_ptr(), p["lin"][i].data_ptr()
        for c in range(3):
            d.shift[c], d.scale[c] = float(self.shift[c]), float(self.scale[c])
        return d


# ---- weights in and out -------------------------------------------------------------------------------------------------------------------
def load_weights(obj_or_path) -> LpipsWeights:
    """A state dict, or a file ``torch.load(..., weights_only=True)`` reads, in one of two key layouts:

      (A) ``lpips.LPIPS(net='alex').state_dict()``: ``net.slice1.0``, ``net.slice2.3``, ``net.slice3.6``, ``net.slice4.8``,
          ``net.slice5.10`` ``.{weight,bias}``; ``lin{0..4}.model.1.weight`` [1,C,1,1] (or ``lins.{i}.model.1.weight``); optional
          ``scaling_layer.{shift,scale}``;
      (B) flat: ``conv{1..5}.{weight,bias}``, ``lin{1..5}`` [C], optional ``shift`` / ``scale`` [3].

    A leading ``module.`` is stripped.  Layout (A) is written from memory of that package, so shapes are checked strictly and a miss names
    the keys looked for and the keys found."""
    sd = obj_or_path
    if not isinstance(sd, Mapping):
        sd = torch.load(obj_or_path, map_location="cpu", weights_only=True)
        if not isinstance(sd, Mapping):
            raise TypeError(f"{obj_or_path}: expected a state dict, got {type(sd).__name__}")
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}

    def pick(names, what):
        for n in names:
            if n in sd:
                return sd[n]
        raise KeyError(f"LPIPS weights: no {what}; looked for {list(names)}, found keys {sorted(sd)}")

    conv_w, conv_b, lin = [], [], []
    for i in range(5):
        conv_w.append(pick((f"conv{i + 1}.weight", _SLICES[i] + ".weight"), f"conv{i + 1} weight"))
        conv_b.append(pick((f"conv{i + 1}.bias", _SLICES[i] + ".bias"), f"conv{i + 1} bias"))
        v = torch.as_tensor(pick((f"lin{i + 1}", f"lin{i}.model.1.weight", f"lins.{i}.model.1.weight"), f"lin{i + 1} weight"))
        if v.dim() == 4:
            if tuple(v.shape) != (1, CHANNELS[i], 1, 1):
                raise ValueError(f"lin{i + 1} has shape {tuple(v.shape)}, (1, {CHANNELS[i]}, 1, 1) or ({CHANNELS[i]},) expected")
            v = v.reshape(-1)
        lin.append(v)

    def opt(names):
        for n in names:
            if n in sd:
                return torch.as_tensor(sd[n]).reshape(-1)
        return None
    return LpipsWeights(conv_w, conv_b, lin, opt(("shift", "scaling_layer.shift")), opt(("scale", "scaling_layer.scale")))


def synth_weights(seed: int = 1234) -> LpipsWeights:
    """Seeded stand-ins at the true widths (one numpy Philox stream per tensor, as utils/synth.synth_state_dict): convolutions and biases
    uniform in +-1/sqrt(fan_in), lin weights uniform in [0,1) (the trained ones are non-negative)."""
    def rng(name):
        return np.random.Generator(np.random.Philox(key=[seed & 0xFFFFFFFF, zlib.crc32(name.encode())]))
    conv_w, conv_b, lin = [], [], []
    for i, (co, ci, k, _, _) in enumerate(CONVS):
        bound = 1.0 / float(ci * k * k) ** 0.5
        conv_w.append(torch.from_numpy(((2.0 * rng(f"conv{i + 1}.weight").random((co, ci, k, k)) - 1.0) * bound).astype(np.float32)))
        conv_b.append(torch.from_numpy(((2.0 * rng(f"conv{i + 1}.bias").random((co,)) - 1.0) * bound).astype(np.float32)))
        lin.append(torch.from_numpy(rng(f"lin{i + 1}").random((co,)).astype(np.float32)))
    return LpipsWeights(conv_w, conv_b, lin)


# ---- the definition in torch ops ----------------------------------------------------------------------------------------------------------
def map_sizes(h: int, w: int) -> List[Tuple[int, int]]:
    """(rows, columns) of the five taps of an ``h`` x ``w`` image."""
    h1, w1 = (h - 7) // 4 + 1, (w - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]


def _check_images(x, name: str) -> None:
    if not isinstance(x, Tensor) or x.dim() != 4:
        raise ValueError(f"{name} must be [N,3,H,W], got {tuple(getattr(x, 'shape', ()))}")
    if x.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"{name} must be uint8 or float32, got {x.dtype}")
    n, c, h, w = x.shape
    if c != 3:
        raise ValueError(f"{name} has {c} channels, RGB expected")
    if n == 0:
        raise ValueError("empty batch")
    if h < MIN_SIZE or w < MIN_SIZE:
        raise ValueError(f"{name} is {h}x{w}: LPIPS (AlexNet) needs at least {MIN_SIZE}x{MIN_SIZE} pixels, the smallest image both max-pools accept")


def _check_pair(a, b) -> None:
    _check_images(a, "a")
    _check_images(b, "b")
    if a.shape != b.shape:
        raise ValueError("Input images must have the same dimensions.")


def _check_weights(weights) -> None:
    if not isinstance(weights, LpipsWeights):
        raise TypeError(f"weights must be LpipsWeights (load_weights / synth_weights), got {type(weights).__name__}")


def quantise_torch(x: Tensor) -> Tensor:
    """uint8 values of an image as float64: a uint8 input as it is, float32 by ``metrics.to_uint8``'s rule (clamp, x 255 in double, round
    half to even, NaN -> 0)."""
    if x.dtype == torch.uint8:
        return x.to(torch.float64)
    x = torch.nan_to_num(x.detach(), nan=0.0, posinf=1.0, neginf=0.0)
    return torch.round(x.clamp(0.0, 1.0).to(torch.float64) * 255.0)


def features_torch(x: Tensor, weights: LpipsWeights, dtype=torch.float32) -> List[Tensor]:
    """The five ReLU taps [N,C_l,h_l,w_l] of images ``x`` (uint8, or float32 in [0,1]) in ``dtype``, on ``x``'s device."""
    _check_images(x, "x")
    _check_weights(weights)
    dev = x.device
    t = (quantise_torch(x).to(dtype) - 127.5) / 127.5
    t = (t - weights.shift.to(dev, dtype).view(1, 3, 1, 1)) / weights.scale.to(dev, dtype).view(1, 3, 1, 1)
    taps = []
    for i, (_, _, _, stride, pad) in enumerate(CONVS):
        if i in (1, 2):
            t = F.max_pool2d(t, kernel_size=3, stride=2)
        t = F.relu(F.conv2d(t, weights.conv_w[i].to(dev, dtype), weights.conv_b[i].to(dev, dtype), stride=stride, padding=pad))
        taps.append(t)
    return taps


def score_torch(f0: List[Tensor], f1: List[Tensor], weights: LpipsWeights) -> Tensor:
    """Steps 4 and 5 on two lists of taps: [N] in the taps' dtype."""
    total = 0
    for a, b, w in zip(f0, f1, weights.lin):
        na = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total = total + ((na - nb).pow(2) * w.to(a.device, a.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))
    return total


def distance_torch(a: Tensor, b: Tensor, weights: LpipsWeights, dtype=torch.float32) -> Tensor:
    """LPIPS of the pairs ``a[i]``, ``b[i]`` by the definition, in ``dtype``, on the inputs' device (CPU included): [N]."""
    _check_pair(a, b)
    with torch.no_grad():
        return score_torch(features_torch(a, weights, dtype), features_torch(b, weights, dtype), weights)


# ---- the device path ----------------------------------------------------------------------------------------------------------------------
def _on_device(x: Tensor, name: str) -> Tensor:
    if not x.is_cuda:
        raise RuntimeError(f"{name} is on {x.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    return x.detach().contiguous()


def _check_size(images: int, h: int, w: int) -> None:
    sizes = map_sizes(h, w)
    largest = max([images * 3 * h * w, images * sizes[1][0] * sizes[1][1] * CHANNELS[0]]
                  + [images * hh * ww * c for (hh, ww), c in zip(sizes, CHANNELS)])
    if largest >= 2 ** 31:
        raise ValueError(f"{images} images of {h}x{w}: the largest tensor of the feature stack would have {largest} elements "
                         f"(limit 2^31 - 1); split the batch")
    if images > 65534:
        raise ValueError(f"{images} images in one call (limit 65534); split the batch")


def _workspace(lib, images: int, pairs: int, h: int, w: int, device) -> Tensor:
    nbytes = lib.virnet_lpips_workspace_bytes(images, pairs, h, w)
    if nbytes == 0:
        _native.check(1, "lpips_workspace_bytes")
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


def distance(a: Tensor, b: Tensor, weights: LpipsWeights) -> Tensor:
    """LPIPS of the pairs ``a[i]``, ``b[i]``: CUDA [N,3,H,W], each uint8 or float32 in the networks' [0,1] scale (clipped and quantised while
    it is read, by ``metrics.to_uint8``'s rule, NaN -> 0).  Returns a float64 device tensor [N].  No synchronisation; enqueues on the current
    stream of the tensors' device; safe inside a caller's graph capture once :meth:`LpipsWeights.prepare` has run for the device."""
    _check_pair(a, b)
    _check_weights(weights)
    n, _, h, w = a.shape
    a, b = _on_device(a, "a"), _on_device(b, "b")
    if a.device != b.device:
        raise RuntimeError(f"a is on {a.device}, b on {b.device}")
    _check_size(2 * n, h, w)
    lib = _native.load()
    with torch.cuda.device(a.device):
        desc = weights._desc(a.device)
        ws = _workspace(lib, 2 * n, n, h, w, a.device)
        out = torch.empty(n, dtype=torch.float64, device=a.device)
        _native.check(lib.virnet_lpips(a.data_ptr(), int(a.dtype == torch.float32), b.data_ptr(), int(b.dtype == torch.float32), n, h, w,
                                       C.byref(desc), ws.data_ptr(), out.data_ptr(), _native.stream_handle()), "lpips")
    return out


def features(x: Tensor, weights: LpipsWeights) -> List[Tensor]:
    """The five ReLU taps of CUDA images ``x`` as float32 NCHW tensors: what :func:`distance` scores, copied out of its NHWC workspace."""
    _check_images(x, "x")
    _check_weights(weights)
    n, _, h, w = x.shape
    x = _on_device(x, "x")
    _check_size(n, h, w)
    lib = _native.load()
    with torch.cuda.device(x.device):
        desc = weights._desc(x.device)
        ws = _workspace(lib, n, 0, h, w, x.device)
        outs = [torch.empty((n, c, hh, ww), dtype=torch.float32, device=x.device) for (hh, ww), c in zip(map_sizes(h, w), CHANNELS)]
        _native.check(lib.virnet_lpips_features(x.data_ptr(), int(x.dtype == torch.float32), n, h, w, C.byref(desc), ws.data_ptr(),
                                                *[o.data_ptr() for o in outs], _native.stream_handle()), "lpips_features")
    return outs


# ---- glue for sisr_eval.sisr_table(device_metrics=True, lpips=weights) --------------------------------------------------------------------
def table_pair(mu: Tensor, gt_hwc: np.ndarray, weights: LpipsWeights) -> Tensor:
    """One image of the table: ``mu`` = the network's un-clipped CUDA output [1,3,H,W] or [3,H,W], ``gt_hwc`` = the uint8 H x W x 3 ground
    truth on the host (uploaded once).  LPIPS is taken on the whole image, no border crop (scripts/sisr_virnet_syn.py:158-161)."""
    if not isinstance(mu, Tensor):
        raise TypeError(f"device_metrics=True: forward must return a CUDA tensor, got {type(mu).__name__}")
    if mu.dim() == 3:
        mu = mu.unsqueeze(0)
    if not mu.is_cuda:
        raise RuntimeError(f"device_metrics=True: forward returned a tensor on {mu.device}; return the network's CUDA output")
    gt = torch.from_numpy(np.ascontiguousarray(gt_hwc.transpose(2, 0, 1)[np.newaxis])).to(mu.device, non_blocking=True)
    return distance(mu, gt, weights)


def table_collect(pending: List[Tensor]) -> List[float]:
    """The per-image LPIPS list of one (dataset, kernel) from its :func:`table_pair` results: ONE synchronisation."""
    return [float(v) for v in torch.cat(pending).cpu().tolist()] if pending else []
