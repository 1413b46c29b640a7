"""Gradient-norm clipping and the Adam step on the device (csrc/optim.hip).

  * :class:`ClipAdam` -- the ``nn.utils.clip_grad_norm_`` calls (one per sub-network) and the ``torch.optim.Adam.step()`` of the reference's
    training loops (train_denoising_syn.py:175-184, train_denoising_real.py:172-177, train_SISR.py:224-229) as one optimizer: one pass over
    the clipped gradients for the norms, one launch that turns them into coefficients on the device, one pass over ``(p, g, m, v)``;
  * :func:`clip_grad_norm_` -- ``nn.utils.clip_grad_norm_`` (2-norm) alone, for callers that keep another optimizer.

CUDA fp32 parameters only, no fallback.  Nothing here synchronises: the calls enqueue on the current stream of the parameters' device, the
norms and the clip coefficients stay on the device, and results are bitwise reproducible (no atomics).  The kernels write parameters
through raw pointers, so :meth:`ClipAdam.step` bumps every stepped parameter's ``_version`` itself: packed weight copies
(networks/params.py), the composed tail (engine.py) and captured graphs (graph.py) follow it as they follow torch's in-place step.

The tensor list of a call is cut into chunks of ``CHUNK`` elements and travels in the kernel arguments, ``TABLE`` tensors per launch
(:func:`plan`); gradients may move every step.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor
from torch.optim import Optimizer

from . import _native

CHUNK = _native.OPTIM_CHUNK          # elements per workgroup
TABLE = _native.OPTIM_TABLE          # tensors per launch


# ---- the plan (host only) ---------------------------------------------------------------------------------------------------------------
def _order(sets: Sequence[int]) -> List[int]:
    """Indices ordered by clip set (stable), tensors in no set (-1) last: a set's chunks are then contiguous."""
    return sorted(range(len(sets)), key=lambda i: (sets[i] < 0, sets[i]))


def _int_array(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def plan(sizes: Sequence[int], sets: Sequence[int], n_sets: Optional[int] = None) -> dict:
    """How a list of tensors with ``sizes`` elements, each in clip set ``sets[i]`` (-1: none), is laid out for the kernels; a pure function
    of its arguments (the library's own planner, no device work).

    ``order``: the tensors' indices as launched (by clip set, no set last); per position of that order ``first_chunk`` (the chunk ordinal
    of the tensor's first chunk; chunk c of a tensor covers its elements [c * CHUNK, min((c + 1) * CHUNK, size))), ``chunks`` and ``table``
    (which launch carries it, at most TABLE tensors each); per set ``set_range``: (first chunk ordinal, chunks) -- the slots of the norm
    pass's fp64 partials."""
    sizes, sets = [int(s) for s in sizes], [int(s) for s in sets]
    if len(sizes) != len(sets):
        raise ValueError(f"{len(sizes)} sizes but {len(sets)} clip sets")
    n_sets = (max(sets) + 1 if sets else 0) if n_sets is None else int(n_sets)
    n_sets = max(n_sets, 0)
    order = _order(sets)
    n = len(order)
    numel = _int_array(C.c_longlong, [sizes[i] for i in order])
    sset = _int_array(C.c_int, [sets[i] for i in order])
    first, table = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
    s_first, s_chunks = (C.c_int * max(n_sets, 1))(), (C.c_int * max(n_sets, 1))()
    _native.check(_native.load().virnet_optim_plan(numel, sset, n, n_sets, first, table, s_first, s_chunks), "optim_plan")
    return {"order": order, "first_chunk": list(first[:n]), "chunks": [-(-sizes[i] // CHUNK) for i in order], "table": list(table[:n]),
            "set_range": [(s_first[s], s_chunks[s]) for s in range(n_sets)]}


# ---- launches (the caller holds torch.cuda.device and no_grad) -------------------------------------------------------------------------
def _ptr_array(tensors: Sequence[Tensor]):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _grad_norms(grads: Sequence[Tensor], sets: Sequence[int], max_norms: Sequence[float], device: torch.device) -> Tensor:
    """fp32 [2][n_sets] on ``device``: the sets' total norms and their clip coefficients.  ``grads`` ordered by set, contiguous fp32."""
    lib = _native.load()
    n, n_sets = len(grads), len(max_norms)
    numel = _int_array(C.c_longlong, [g.numel() for g in grads])
    sset = _int_array(C.c_int, sets)
    ws = torch.empty(lib.virnet_optim_workspace_bytes(numel, sset, n) // 8, dtype=torch.float64, device=device)
    out = torch.empty((2, n_sets), dtype=torch.float32, device=device)
    _native.check(lib.virnet_optim_grad_norms(_ptr_array(grads), numel, sset, n, _int_array(C.c_float, list(max_norms)), n_sets, ws.data_ptr(),
                                              out.data_ptr(), out.data_ptr() + 4 * n_sets, _native.stream_handle()), "optim_grad_norms")
    return out


def _max_norm(v) -> float:
    if isinstance(v, (bool, Tensor)) or not isinstance(v, (int, float)) or math.isnan(float(v)) or float(v) < 0.0:
        raise ValueError(f"max_norm {v!r}: a non-negative float is expected")
    return float(v)


def _check_param(p, what: str = "parameter") -> None:
    if not isinstance(p, Tensor):
        raise TypeError(f"{what} must be a tensor, got {type(p).__name__}")
    if p.dtype != torch.float32:
        raise TypeError(f"{what} {tuple(p.shape)} is {p.dtype}: the device optimizer takes float32 parameters only")
    if p.is_sparse or p.layout != torch.strided:
        raise TypeError(f"{what} {tuple(p.shape)} is not a dense strided tensor")
    if not p.is_contiguous():
        raise ValueError(f"{what} {tuple(p.shape)} is not contiguous: the kernels update parameters in place through one flat range")
    if p.numel() >= 1 << 31:
        raise ValueError(f"{what} {tuple(p.shape)} has {p.numel()} elements (below 2^31 expected)")


def _dense_grad(p: Tensor, device: torch.device) -> Tuple[Tensor, bool]:
    """(the gradient as a contiguous fp32 tensor on ``device``, whether that is a copy)"""
    g = p.grad
    if g.is_sparse or g.layout != torch.strided:
        raise RuntimeError("sparse gradients are not supported")
    if g.dtype != torch.float32 or g.device != device or g.shape != p.shape:
        raise RuntimeError(f"gradient {tuple(g.shape)} {g.dtype} on {g.device} does not match its parameter {tuple(p.shape)} float32 on {device}")
    if g.is_contiguous():
        return g, False
    return g.contiguous(), True


def _require_cuda(p: Tensor, who: str) -> None:
    if not p.is_cuda:
        raise RuntimeError(f"{who}: parameter {tuple(p.shape)} is on {p.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")


def clip_grad_norm_(parameters: Union[Tensor, Iterable[Tensor]], max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False,
                    foreach=None) -> Tensor:
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` for the 2-norm on the device: scales the gradients in place by
    ``min(max_norm / (total_norm + 1e-6), 1)`` and returns the total norm as a 0-dim fp32 CUDA tensor, without a host sync.  The norm is
    the fp32 rounding of an fp64 sum.  ``error_if_nonfinite=True`` would need that sync and is refused; a non-finite norm propagates into
    the gradients as it does in torch.  Parameters without a gradient are skipped."""
    if isinstance(parameters, Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if float(norm_type) != 2.0:
        raise ValueError(f"norm_type {norm_type!r}: only the 2-norm runs on the device")
    if error_if_nonfinite:
        raise ValueError("error_if_nonfinite=True needs a host synchronisation; test the returned norm instead")
    max_norm = _max_norm(max_norm)
    if not params:
        return torch.tensor(0.0)
    for p in params:
        if p.dtype != torch.float32:
            raise TypeError(f"parameter {tuple(p.shape)} is {p.dtype}: float32 expected")
        _require_cuda(p, "clip_grad_norm_")
    device = params[0].device
    if any(p.device != device for p in params):
        raise RuntimeError("clip_grad_norm_: the parameters are on more than one device")
    with torch.no_grad(), torch.cuda.device(device):
        grads, copies = [], []
        for p in params:
            if p.grad.numel() == 0:
                continue
            g, copied = _dense_grad(p, device)
            grads.append(g)
            if copied:
                copies.append((p.grad, g))
        if not grads:
            return torch.zeros((), dtype=torch.float32, device=device)
        sets = [0] * len(grads)
        out = _grad_norms(grads, sets, [max_norm], device)
        _native.check(_native.load().virnet_optim_scale_grads(_ptr_array(grads), _int_array(C.c_longlong, [g.numel() for g in grads]),
                                                              _int_array(C.c_int, sets), len(grads), 1, out.data_ptr() + 4,
                                                              _native.stream_handle()), "optim_scale_grads")
        for dst, src in copies:
            dst.copy_(src)
    return out[0, 0]


# ---- the optimizer -----------------------------------------------------------------------------------------------------------------------
class ClipAdam(Optimizer):
    """``torch.optim.Adam`` with the per-sub-network ``clip_grad_norm_`` calls folded in, on the kernels of csrc/optim.hip.

        opt = ClipAdam(net.parameters(), lr=1e-4, clip=[(params_R, 1e3), (params_S, 1e2)])
        opt.zero_grad(); loss.backward(); opt.step()
        norm_R, norm_S = opt.grad_norms        # fp32 CUDA tensor [len(clip)]: the pre-clip norms; reading it is the caller's sync

    ``lr``, ``betas``, ``eps``, ``weight_decay`` as ``torch.optim.Adam`` (L2 weight decay; ``lr`` a Python float, read from ``param_groups``
    at every step, so schedulers work unchanged).  ``clip``: (parameters, max_norm) pairs, independent of the parameter groups; a parameter is
    in at most one set and may be in none (it is then stepped with its gradient as it is); a member of a set must be in a parameter group
    by the time of the first step (``ValueError`` otherwise: its gradient would silently be missing from the set's norm).  ``write_back_grads=True`` also writes the
    clipped gradients to ``p.grad`` -- what the reference's in-place clip leaves behind; off by default (4 bytes per parameter less).
    ``grad_norms`` and ``clip_coefs`` hold the last step's norms and coefficients on the device (None before the first step, and after a step
    in which no parameter had a gradient).

    State layout and ``defaults`` are ``torch.optim.Adam``'s (per parameter ``step`` as a CPU fp32 scalar, ``exp_avg``, ``exp_avg_sq``): a
    ``state_dict()`` of either loads into the other.  ``amsgrad``, ``maximize``, ``decoupled_weight_decay`` and parameters that are not
    contiguous fp32 are refused.  CPU parameters can be constructed with and take ``load_state_dict``; ``step()`` raises on them."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, clip: Iterable[Tuple[Iterable[Tensor], float]] = (), write_back_grads: bool = False,
                 maximize: bool = False, decoupled_weight_decay: bool = False):
        if isinstance(lr, (bool, Tensor)) or not isinstance(lr, (int, float)) or not 0.0 <= lr:
            raise ValueError(f"lr {lr!r}: a non-negative Python float is expected (it travels as a kernel argument)")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=decoupled_weight_decay)
        self.write_back_grads = bool(write_back_grads)
        self.grad_norms: Optional[Tensor] = None
        self.clip_coefs: Optional[Tensor] = None
        self.clip_sets: List[Tuple[List[Tensor], float]] = []
        super().__init__(params, defaults)
        seen: Dict[int, int] = {}
        for s, (members, max_norm) in enumerate(clip):
            members = [members] if isinstance(members, Tensor) else list(members)
            for p in members:
                _check_param(p, f"clip set {s}: parameter")
                if id(p) in seen:
                    raise ValueError(f"parameter {tuple(p.shape)} is in clip sets {seen[id(p)]} and {s}: a parameter is in at most one set")
                seen[id(p)] = s
            self.clip_sets.append((members, _max_norm(max_norm)))

    def __getstate__(self):
        # (Optimizer pickles defaults, state and param_groups only: copy.deepcopy(opt) must keep the clip sets)
        state = super().__getstate__()
        state.update(clip_sets=self.clip_sets, write_back_grads=self.write_back_grads, grad_norms=self.grad_norms, clip_coefs=self.clip_coefs)
        return state

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    @staticmethod
    def _check_group(group) -> None:
        for key in ("amsgrad", "maximize", "decoupled_weight_decay", "capturable", "differentiable"):
            if group.get(key):
                raise ValueError(f"ClipAdam: {key}=True is not supported by the device step")
        if isinstance(group["lr"], Tensor):
            raise ValueError("ClipAdam: lr must be a Python float (it travels as a kernel argument)")
        for p in group["params"]:
            _check_param(p)

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
            group["foreach"], group["fused"] = None, None          # (a checkpoint of Adam(fused=True) keeps its step counts on the device)
        for st in self.state.values():
            step = st.get("step")
            if isinstance(step, Tensor) and (step.device.type != "cpu" or step.dtype != torch.float32):
                st["step"] = step.detach().to("cpu", torch.float32)

    def _set_of(self) -> Dict[int, int]:
        return {id(p): s for s, (members, _) in enumerate(self.clip_sets) for p in members}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        set_of = self._set_of()
        grouped = {id(p) for group in self.param_groups for p in group["params"]}
        for s, (members, _) in enumerate(self.clip_sets):
            for p in members:
                if id(p) not in grouped:
                    raise ValueError(f"clip set {s}: parameter {tuple(p.shape)} is in no parameter group; clip_grad_norm_ would count its gradient, "
                                     f"this optimizer only sees the parameters it steps")
        per_device: Dict[torch.device, list] = {}
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            for p in group["params"]:
                _require_cuda(p, "ClipAdam.step")
                if p.grad is None or p.numel() == 0:
                    continue
                per_device.setdefault(p.device, []).append((set_of.get(id(p), -1), gi, p))
        if len(per_device) > 1 and self.clip_sets:
            raise RuntimeError("ClipAdam.step: the parameters are on more than one device; a clip set's norm is formed on one")
        self.grad_norms = self.clip_coefs = None
        for device, items in per_device.items():
            with torch.cuda.device(device):
                self._step_device(device, items)
        return loss

    def _step_device(self, device: torch.device, items: list) -> None:
        lib = _native.load()
        stream = _native.stream_handle()
        n_sets = len(self.clip_sets)
        items.sort(key=lambda it: (it[0] < 0, it[0], it[1]))          # by clip set, no set last (stable: then by group)
        keep = []                                                       # contiguous copies of gradients stay alive until every launch is enqueued
        grads = []
        for _, _, p in items:
            g, copied = _dense_grad(p, device)
            grads.append(g)
            if copied:
                keep.append((p.grad, g))
        coef_ptr = 0
        if n_sets:
            in_sets = sum(1 for it in items if it[0] >= 0)
            out = _grad_norms(grads[:in_sets], [it[0] for it in items[:in_sets]], [m for _, m in self.clip_sets], device)
            self.grad_norms, self.clip_coefs = out[0], out[1]
            coef_ptr = out.data_ptr() + 4 * n_sets
        consts: Dict[tuple, Tuple[float, float]] = {}
        for gi, group in enumerate(self.param_groups):
            idx = [k for k, it in enumerate(items) if it[1] == gi]
            if not idx:
                continue
            lr, (beta1, beta2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
            ps, gs, ms, vs, sets, step_size, bc2 = [], [], [], [], [], [], []
            for k in idx:
                s, _, p = items[k]
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                for name, t in (("exp_avg", m), ("exp_avg_sq", v)):
                    if t.dtype != torch.float32 or t.device != device or t.shape != p.shape or not t.is_contiguous():
                        raise RuntimeError(f"ClipAdam.step: state {name} {tuple(t.shape)} {t.dtype} on {t.device} does not match its parameter "
                                           f"{tuple(p.shape)} float32 on {device}")
                t_ = float(st["step"]) + 1.0                           # (the count itself moves once the launch has been accepted)
                key = (t_, lr, beta1, beta2)
                if key not in consts:
                    # torch's single-tensor path in Python doubles, each rounded once to fp32 on the way into the kernel
                    consts[key] = (lr / (1.0 - beta1 ** t_), math.sqrt(1.0 - beta2 ** t_))
                ps.append(p); gs.append(grads[k]); ms.append(m); vs.append(v); sets.append(s)
                step_size.append(consts[key][0]); bc2.append(consts[key][1])
            _native.check(lib.virnet_optim_adam_step(_ptr_array(ps), _ptr_array(gs), _ptr_array(ms), _ptr_array(vs),
                                                     _int_array(C.c_longlong, [p.numel() for p in ps]), _int_array(C.c_int, sets),
                                                     _int_array(C.c_float, step_size), _int_array(C.c_float, bc2), len(ps), n_sets, coef_ptr,
                                                     1.0 - beta1, beta2, 1.0 - beta2, eps, wd, int(self.write_back_grads), stream), "optim_adam_step")
            for p in ps:
                self.state[p]["step"] += 1
        if self.write_back_grads:
            for dst, src in keep:
                dst.copy_(src)
        # the kernels wrote through raw pointers: tell autograd, the packed weight copies and the captured graphs
        torch.autograd.graph.increment_version([p for _, _, p in items])


def __getattr__(name: str):
    # ``optim.WeightEMA``: the weight average lives next to the optimizer (ema.py imports this module, hence the late import)
    if name == "WeightEMA":
        from .ema import WeightEMA
        return WeightEMA
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
