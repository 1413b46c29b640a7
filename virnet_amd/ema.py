"""Exponential moving average of the weights on the device (csrc/ema.hip).

    ema = WeightEMA(net, decay=0.999, warmup=False)     # or an iterable of (name, parameter)
    opt.step(); ema.update()                            # one launch per TABLE tensors, no host sync
    with ema.averaged():                                # swap in, ..., swap back
        psnr = validate(net, val)
    ema.swap()                                          # the bare exchange
    ema.model_state_dict()                              # clones of the averages under the model's state_dict keys
    ema.state_dict() / ema.load_state_dict(sd)          # {"decay", "warmup", "num_updates", "shadow": {name: tensor}}

The averages live in SHADOW TENSORS, one per parameter, not in a shadow module: a second module would carry its own packed weights, its own
composed tail and its own captured graphs (and ``copy.deepcopy`` of a network that has run an eval forward raises).  To run the network on
the averages they are exchanged with the parameters in place (:meth:`WeightEMA.swap`), after which every swapped parameter's ``_version``
is bumped, so packed weight copies (networks/params.py), the composed tail (engine.py) and captured graphs (graph.py) follow as they
follow :meth:`optim.ClipAdam.step`.  Nothing is tied to ``ClipAdam``: any optimizer may step the parameters.

An update is ``e = e + w (p - e)`` with ``w = float32(1 - decay_at(t))``, three fp32 operations each rounded on its own (:func:`ema_np` is
the definition); ``t`` counts the updates already made and is a Python int, so there is no device counter and nothing synchronises.
CUDA fp32 parameters only, no fallback; a CPU module can be constructed with and can load state.
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager
from typing import Dict, Iterable, List, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _native
from .optim import _check_param, _int_array, _ptr_array, _require_cuda


def decay_at(t: int, decay: float, warmup: bool = False) -> float:
    """The decay of the update after ``t`` updates have been made: ``decay``, or with ``warmup`` ``min(decay, (1 + t) / (10 + t))`` (the
    average follows the first steps closely instead of remembering the initial weights).  Python doubles."""
    if not warmup:
        return float(decay)
    return min(float(decay), (1.0 + t) / (10.0 + t))


def weight_at(t: int, decay: float, warmup: bool = False) -> float:
    """The update's weight: ``1 - decay_at(t)`` formed in doubles and rounded once to fp32 (returned as the Python float of that fp32)."""
    return float(np.float32(1.0 - decay_at(t, decay, warmup)))


def ema_np(e: np.ndarray, p: np.ndarray, w) -> np.ndarray:
    """The update as the kernel does it, on float32 arrays: ``d = p - e; t = w * d; e + t``, each a float32 operation."""
    e, p, w = np.asarray(e), np.asarray(p), np.float32(w)
    if e.dtype != np.float32 or p.dtype != np.float32:
        raise TypeError(f"ema_np takes float32 arrays, got {e.dtype} and {p.dtype}")
    d = np.subtract(p, e, dtype=np.float32)
    t = np.multiply(w, d, dtype=np.float32)
    return np.add(e, t, dtype=np.float32)


def _check_decay(decay) -> float:
    if isinstance(decay, (bool, Tensor)) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
        raise ValueError(f"decay {decay!r}: a Python float with 0 <= decay < 1 is expected")
    return float(decay)


class WeightEMA:
    """See the module docstring.  ``model``: a module (its ``named_parameters()``; the networks have no buffers) or an iterable of
    (name, parameter).  ``names``, ``params`` and ``shadows`` are parallel lists; the shadows are clones of the parameters at
    construction.  ``num_updates``: updates made so far; ``swapped``: the parameters currently hold the averages (and the shadows the
    live weights)."""

    def __init__(self, model: Union[torch.nn.Module, Iterable[Tuple[str, Tensor]]], decay: float = 0.999, warmup: bool = False):
        self.decay = _check_decay(decay)
        self.warmup = bool(warmup)
        named = list(model.named_parameters()) if isinstance(model, torch.nn.Module) else list(model)
        self.names: List[str] = []
        self.params: List[Tensor] = []
        for item in named:
            if not isinstance(item, (tuple, list)) or len(item) != 2 or not isinstance(item[0], str):
                raise TypeError("WeightEMA takes a module or an iterable of (name, parameter) pairs")
            name, p = item
            _check_param(p, f"parameter {name}")
            if name in self.names:
                raise ValueError(f"parameter name {name!r} appears twice")
            if p.numel() == 0:
                continue
            self.names.append(name)
            self.params.append(p)
        with torch.no_grad():
            self.shadows: List[Tensor] = []
            for p in self.params:
                s = torch.empty_like(p, memory_format=torch.contiguous_format)
                s.copy_(p.detach())
                self.shadows.append(s)
        self.num_updates = 0
        self.swapped = False
        self._cached_groups = None

    # ---- launches ------------------------------------------------------------------------------------------------------------------------
    def _groups(self, who: str) -> list:
        """Per device of the parameters: (device, count, shadow pointers, parameter pointers, numel) as the C arrays of a launch.  Every
        call reads every tensor's address; the checks and the arrays are redone only when an address has changed (a ``Module.to``, a
        rebound ``.data``): an unchanged address is the same storage on the same device."""
        where = ([s.data_ptr() for s in self.shadows], [p.data_ptr() for p in self.params])
        if self._cached_groups is not None and self._cached_groups[0] == where:
            return self._cached_groups[1]
        per_device: Dict[torch.device, List[int]] = {}
        for i, (p, s) in enumerate(zip(self.params, self.shadows)):
            _require_cuda(p, who)
            if s.device != p.device or s.shape != p.shape or not s.is_contiguous() or s.dtype != torch.float32:
                raise RuntimeError(f"{who}: shadow {self.names[i]} is {tuple(s.shape)} {s.dtype} on {s.device}, its parameter {tuple(p.shape)} "
                                   f"float32 on {p.device}")
            _check_param(p, f"parameter {self.names[i]}")
            per_device.setdefault(p.device, []).append(i)
        groups = [(device, len(idx), _ptr_array([self.shadows[i] for i in idx]), _ptr_array([self.params[i] for i in idx]),
                   _int_array(C.c_longlong, [self.params[i].numel() for i in idx])) for device, idx in per_device.items()]
        self._cached_groups = (where, groups)
        return groups

    def _launch(self, who: str, entry, *scalars) -> None:
        for device, count, shadows, params, numel in self._groups(who):
            with torch.cuda.device(device):
                _native.check(entry(shadows, params, numel, count, *scalars, _native.stream_handle()), who)

    def decay_at(self, t: int = None) -> float:
        """:func:`decay_at` with this average's settings, by default at its own count."""
        return decay_at(self.num_updates if t is None else t, self.decay, self.warmup)

    @torch.no_grad()
    def update(self) -> None:
        """``shadow = shadow + w (parameter - shadow)`` for every parameter, ``w = float32(1 - decay_at(num_updates))``; enqueues on the
        current stream of the parameters' device and returns."""
        if self.swapped:
            raise RuntimeError("WeightEMA.update: the averaged weights are swapped in; swap back before the next update")
        w = weight_at(self.num_updates, self.decay, self.warmup)
        self._launch("WeightEMA.update", _native.load().virnet_ema_update, w)
        self.num_updates += 1

    @torch.no_grad()
    def swap(self) -> None:
        """Exchange the parameters with their shadows, bit for bit, and bump the parameters' ``_version``."""
        self._launch("WeightEMA.swap", _native.load().virnet_ema_swap)
        # the kernel wrote through raw pointers: tell autograd, the packed weight copies and the captured graphs
        if self.params:
            torch.autograd.graph.increment_version(self.params)
        self.swapped = not self.swapped

    @contextmanager
    def averaged(self):
        """Inside the block the parameters hold the averages; the live weights come back on leaving, also after an exception."""
        if self.swapped:
            raise RuntimeError("WeightEMA.averaged: the averaged weights are already swapped in")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # ---- state ---------------------------------------------------------------------------------------------------------------------------
    def _averages(self) -> List[Tensor]:
        return self.params if self.swapped else self.shadows

    def checksum(self) -> Tensor:
        """One fp64 sum over all averages, formed on their device (the multi-rank loops compare it across ranks)."""
        with torch.no_grad():
            return torch.cat([s.detach().reshape(-1) for s in self._averages()]).double().sum().reshape(1)

    def model_state_dict(self) -> Dict[str, Tensor]:
        """Clones of the averages under the model's ``state_dict`` keys: loadable into a fresh module (``fit.load_model_state``)."""
        return {name: s.detach().clone() for name, s in zip(self.names, self._averages())}

    def state_dict(self) -> dict:
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates, "shadow": self.model_state_dict()}

    def load_state_dict(self, sd: dict) -> None:
        """Restore ``state_dict()``'s form (the tensors are copied to the shadows' device).  A ``module.`` prefix on every key of
        ``shadow`` is accepted, as ``fit.load_model_state`` accepts it."""
        if self.swapped:
            raise RuntimeError("WeightEMA.load_state_dict: the averaged weights are swapped in; swap back first")
        for key in ("decay", "warmup", "num_updates", "shadow"):
            if key not in sd:
                raise KeyError(f"EMA state lacks {key!r}")
        shadow = sd["shadow"]
        if shadow and all(k.startswith("module.") for k in shadow):
            shadow = {k[len("module."):]: v for k, v in shadow.items()}
        missing, extra = [n for n in self.names if n not in shadow], [k for k in shadow if k not in set(self.names)]
        if missing or extra:
            raise KeyError(f"EMA state: missing shadow(s) {missing}, unexpected {extra}")
        decay, count = _check_decay(sd["decay"]), sd["num_updates"]
        if isinstance(count, bool) or int(count) != count or int(count) < 0:
            raise ValueError(f"EMA state: num_updates {count!r}: a non-negative integer is expected")
        for name, s in zip(self.names, self.shadows):
            src = shadow[name]
            if not isinstance(src, Tensor) or src.shape != s.shape or src.dtype != torch.float32:
                raise ValueError(f"EMA state: shadow {name} is {tuple(getattr(src, 'shape', ()))} {getattr(src, 'dtype', type(src).__name__)}, "
                                 f"{tuple(s.shape)} float32 expected")
        with torch.no_grad():
            for name, s in zip(self.names, self.shadows):
                s.copy_(shadow[name])
        self.decay, self.warmup, self.num_updates = decay, bool(sd["warmup"]), int(count)
