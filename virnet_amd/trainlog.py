"""The per-step scalars of a training loop, kept on the device until the loop prints (csrc/trainlog.hip).

The reference reads four ``.item()`` values and two gradient norms on EVERY step (train_denoising_syn.py:186-198): six host stalls per
step for a line it prints every ``print_freq`` steps.  :class:`StepLog` takes the same scalars as device tensors instead:

    log = StepLog(["Loss", "lh", "KLG", "KLIG", "GNorm_R", "GNorm_S"], capacity=128, num_iter=steps_per_epoch)
    log.push(loss, lh, kl_g, kl_ig, opt.grad_norms)        # every step: one launch, no host sync
    rows, sums = log.read()                                # when the loop prints: the only synchronisation

CUDA fp32 tensors only, no fallback.  ``push`` enqueues on the current stream of the log's device; the tensors' device pointers travel in
the kernel arguments, so nothing is uploaded.  The running sums are the reference's ``loss_per_epoch[...] += x.item() / num_iter``
(:187-190) bit for bit: one thread per value adds ``double(x) / double(num_iter)`` in step order.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _native

MAX_VALUES = _native.TRAINLOG_MAX
MAX_CAPACITY = _native.TRAINLOG_MAX_CAPACITY


class StepLog:
    """``StepLog(names, capacity, num_iter, device="cuda")``: ``names`` one per value of a step (``k = len(names)`` <= 16); ``capacity`` rows
    of the device ring (at most that many steps may lie between two reads); ``num_iter`` the divisor of the running sums (the reference's
    ``num_iter_epoch['train']``).

    :meth:`push` takes the step's device scalars -- 0-dim tensors and 1-D tensors such as ``ClipAdam.grad_norms``, ``k`` values in all, in
    the order of ``names`` -- and writes them to slot ``step % capacity`` of the ring and into the sums, in one launch.  :meth:`read` is the
    only synchronisation: one non-blocking copy of sums and ring into pinned memory plus an event wait; it returns the rows pushed since
    the last read (float32 [m, k], oldest first) and the sums (float64 [k]).  :meth:`reset` zeroes the sums on the stream (a new epoch).
    The device buffers are allocated at the first push."""

    def __init__(self, names: Sequence[str], capacity: int, num_iter: int, device="cuda"):
        names = [names] if isinstance(names, str) else list(names)
        if not names or not all(isinstance(s, str) for s in names):
            raise TypeError("StepLog: names must be a non-empty list of strings, one per value of a step")
        if len(names) > MAX_VALUES:
            raise ValueError(f"StepLog: names holds {len(names)} values, at most {MAX_VALUES} per step are supported")
        for what, v, hi in (("capacity", capacity, MAX_CAPACITY), ("num_iter", num_iter, (1 << 31) - 1)):
            if isinstance(v, (bool, Tensor)) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= hi:
                raise ValueError(f"StepLog: {what} {v!r}: an integer 1..{hi} is expected")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"StepLog: device {dev}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
        self.names: List[str] = names
        self.k, self.capacity, self.num_iter = len(names), int(capacity), int(num_iter)
        self._device_arg = dev
        self.device: Optional[torch.device] = dev if dev.index is not None else None          # (resolved at the first push)
        self.pushed = 0           # steps pushed so far
        self.read_mark = 0        # steps the host has read
        self._buf: Optional[Tensor] = None
        self._host: Optional[Tensor] = None
        self._event = None

    # ---- checks (host only) ----------------------------------------------------------------------------------------------------------
    def _same_device(self, d: torch.device) -> bool:
        if self.device is not None:
            return d == self.device
        return d.type == "cuda"

    def _check_push(self, tensors) -> Tuple[List[Tensor], List[int]]:
        if not tensors:
            raise ValueError(f"StepLog.push: no tensors given, {self.k} values ({', '.join(self.names)}) expected")
        counts, covers, first = [], [], 0
        for i, t in enumerate(tensors):          # what each argument is, in order ...
            if not isinstance(t, Tensor):
                raise TypeError(f"StepLog.push: argument {i} must be a tensor, got {type(t).__name__}")
            if t.dim() > 1:
                raise ValueError(f"StepLog.push: argument {i} has shape {tuple(t.shape)}: 0-dim and 1-D tensors are expected")
            cnt = int(t.numel())
            if cnt < 1:
                raise ValueError(f"StepLog.push: argument {i} is empty")
            if first + cnt > self.k:
                raise ValueError(f"StepLog.push: argument {i} brings the step to {first + cnt} values, the log holds k = {self.k} "
                                 f"({', '.join(self.names)}; at most {MAX_VALUES})")
            covers.append(", ".join(repr(s) for s in self.names[first:first + cnt]))
            if t.dtype != torch.float32:
                raise TypeError(f"StepLog.push: argument {i} ({covers[i]}) is {t.dtype}: float32 is expected")
            if cnt > 1 and t.stride(0) != 1:
                raise ValueError(f"StepLog.push: argument {i} ({covers[i]}) is not contiguous")
            counts.append(cnt)
            first += cnt
        if first != self.k:
            raise ValueError(f"StepLog.push: the arguments hold {first} values, the log k = {self.k} ({', '.join(self.names)})")
        for i, t in enumerate(tensors):          # ... then where it lives
            if not t.is_cuda:
                raise RuntimeError(f"StepLog.push: argument {i} ({covers[i]}) is on {t.device}: the VIRNet HIP path runs on a ROCm device only "
                                   f"(no CPU fallback)")
            if not self._same_device(t.device):
                raise RuntimeError(f"StepLog.push: argument {i} ({covers[i]}) is on {t.device}, the log on {self.device}")
        if self.pushed - self.read_mark >= self.capacity:
            raise RuntimeError(f"StepLog.push: step {self.pushed} would overwrite slot {self.pushed % self.capacity}, which holds step "
                               f"{self.pushed - self.capacity} and has not been read (capacity {self.capacity}): call read() first")
        return [t.detach() for t in tensors], counts

    # ---- device ------------------------------------------------------------------------------------------------------------------------
    def _allocate(self, device: torch.device) -> None:
        lib = _native.load()
        nbytes = lib.virnet_trainlog_bytes(self.k, self.capacity)
        if nbytes == 0:
            _native.check(1, "trainlog_bytes")
        self.device = device
        with torch.cuda.device(device):
            self._buf = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)          # (fp64 sums first: the storage is 256-byte aligned)
            with _native.capture_lock:      # (pinned allocation is not permitted while any stream of the process captures)
                self._host = torch.zeros(nbytes // 4, dtype=torch.float32, pin_memory=True)
            self._event = torch.cuda.Event()

    def push(self, *tensors: Tensor) -> None:
        ts, counts = self._check_push(tensors)
        if self._buf is None:
            self._allocate(ts[0].device)
        with torch.no_grad(), torch.cuda.device(self.device):
            src = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            cnt = (C.c_int * len(ts))(*counts)
            _native.check(_native.load().virnet_trainlog_push(src, cnt, len(ts), self._buf.data_ptr(), self.k, self.capacity,
                                                              self.pushed % self.capacity, self.num_iter, _native.stream_handle()), "trainlog_push")
        self.pushed += 1

    def reset(self) -> None:
        """Zero the running sums on the current stream (rows not yet read stay readable)."""
        if self._buf is None:
            return
        with torch.cuda.device(self.device):
            _native.check(_native.load().virnet_trainlog_reset(self._buf.data_ptr(), self.k, _native.stream_handle()), "trainlog_reset")

    def read(self) -> Tuple[np.ndarray, np.ndarray]:
        """(rows float32 [m, k] pushed since the last read, oldest first; sums float64 [k]).  The only synchronisation of the log."""
        if self._buf is None:
            return np.zeros((0, self.k), dtype=np.float32), np.zeros(self.k, dtype=np.float64)
        with torch.cuda.device(self.device):
            self._host.copy_(self._buf, non_blocking=True)
            self._event.record()
            self._event.synchronize()
        flat = self._host.numpy()
        sums = flat[:2 * self.k].view(np.float64).copy()
        ring = flat[2 * self.k:].reshape(self.capacity, self.k)
        rows = np.stack([ring[s % self.capacity] for s in range(self.read_mark, self.pushed)]) if self.pushed > self.read_mark \
            else np.zeros((0, self.k), dtype=np.float32)
        self.read_mark = self.pushed
        return rows.copy(), sums
