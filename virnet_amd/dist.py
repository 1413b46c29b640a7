"""Multi-GPU plumbing: one process per GPU, images sharded, weights broadcast once; for training, bucketed gradient averaging.

The path shards by independent images (no batch statistics, no cross-sample op -- SURVEY.md 8e), so the only collective
is ONE flat fp32 weight broadcast at start-up (42 MB for the denoise-syn net).  On ROCm ``backend="nccl"`` is RCCL; on the
fully connected xGMI mesh rank 0 feeds its 7 peers over 7 distinct links.  There is no per-image communication.
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, List, Optional, Tuple

import torch
import torch.distributed as dist

from . import _native


def env_rank() -> Tuple[int, int, int]:
    """(rank, local_rank, world_size) from the torchrun environment (1-process defaults otherwise)."""
    return int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))


def init(backend: Optional[str] = None, timeout=None) -> Tuple[int, int, int]:
    """Join the process group of the torchrun environment (a no-op for one process).  ``timeout``: seconds or a ``timedelta`` after which a
    collective whose peer never arrives fails -- a dead rank then ends its peers instead of parking them for the backend's default."""
    rank, local_rank, world = env_rank()
    extra = {}
    if timeout is not None:
        import datetime
        extra["timeout"] = timeout if isinstance(timeout, datetime.timedelta) else datetime.timedelta(seconds=float(timeout))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend is None:
            backend = os.environ.get("VIRNET_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if torch.cuda.is_available():
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
        dist.init_process_group(backend=backend, init_method="env://", rank=rank, world_size=world, **extra)
    return rank, local_rank, world


def shard_range(total: int, world: int, rank: int) -> Tuple[int, int]:
    """Images [start, stop) of rank ``rank``: contiguous, sizes differ by at most one, every image owned exactly once."""
    if total < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"bad shard request total={total} world={world} rank={rank}")
    base, rem = divmod(total, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


@torch.no_grad()
def broadcast_parameters(module: torch.nn.Module, src: int = 0, group=None) -> int:
    """Replace every parameter/buffer by rank ``src``'s values with ONE collective over a flat fp32 buffer.

    Returns the number of bytes broadcast.  A no-op (0) when torch.distributed is not initialised."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return 0
    tensors = list(module.state_dict().values())
    if not tensors:
        return 0
    flat = torch.cat([t.detach().reshape(-1).float() for t in tensors])
    dist.broadcast(flat, src=src, group=group)
    off = 0
    for t in tensors:
        n = t.numel()
        t.copy_(flat[off:off + n].view_as(t))   # in-place: bumps ._version, so packed weights are rebuilt
        off += n
    return flat.numel() * 4


def rank_topology(seen, world: int) -> dict:
    """``seen`` = one ``(device uuid, devices visible to that rank)`` pair per rank.  Returns the topology block of the benchmark line and
    raises when two ranks share a device ALTHOUGH every rank sees at least ``world`` devices -- a launcher that hides devices per rank or a
    wrong LOCAL_RANK must not produce a "scaling" number (fewer devices than ranks is the declared rehearsal mode of a 1-GPU box).
    Reference launch pattern: train_denoising_syn.py:280-297 (one process per visible GPU)."""
    uuids, counts = [u for u, _ in seen], [int(c) for _, c in seen]
    if len(seen) != world:
        raise ValueError(f"rank_topology: {len(seen)} reports for {world} ranks")
    topo = {"ranks": world, "ranks_seen": len(set(uuids)), "devices_visible_per_rank": counts, "uuids": uuids}
    if topo["ranks_seen"] < world and min(counts) >= world:
        raise RuntimeError(f"{world} ranks landed on {topo['ranks_seen']} distinct devices although every rank sees >= {world} devices ({uuids}): "
                           "refusing to report a multi-GPU number (check LOCAL_RANK / HIP_VISIBLE_DEVICES)")
    return topo


def max_over_ranks(value: float, device: Optional[torch.device] = None) -> float:
    """MAX all-reduce of a python float (the benchmark's wall time)."""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return value
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def gather_shards(local: torch.Tensor, total: int) -> Optional[torch.Tensor]:
    """Optional result collection: all ranks receive the full [total, ...] batch (excluded from images/s)."""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return local
    world = dist.get_world_size()
    sizes = [shard_range(total, world, r) for r in range(world)]
    mx = max(b - a for a, b in sizes)
    pad = torch.zeros((mx,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    outs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(outs, pad)
    return torch.cat([o[: b - a] for o, (a, b) in zip(outs, sizes)], 0)


# ---- gradient buckets on the device (csrc/gradsync.hip) -------------------------------------------------------------------------------
GRADSYNC_CHUNK = _native.GRADSYNC_CHUNK         # elements per workgroup
GRADSYNC_TABLE = _native.GRADSYNC_TABLE         # tensors per launch


def _check_bucket(bucket, who: str) -> None:
    if not isinstance(bucket, torch.Tensor):
        raise TypeError(f"{who}: bucket must be a tensor, got {type(bucket).__name__}")
    if bucket.dtype != torch.float32:
        raise TypeError(f"{who}: bucket is {bucket.dtype}: the gradient buckets are float32 only")
    if not bucket.is_cuda:
        raise RuntimeError(f"{who}: bucket is on {bucket.device}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
    if bucket.dim() != 1 or not bucket.is_contiguous():
        raise ValueError(f"{who}: bucket {tuple(bucket.shape)} is not a flat contiguous tensor")


def _check_member(t, i: int, bucket: torch.Tensor, who: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: tensor {i} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: tensor {i} {tuple(t.shape)} is {t.dtype}: the gradient buckets take float32 tensors only")
    if t.is_sparse or t.layout != torch.strided:
        raise TypeError(f"{who}: tensor {i} {tuple(t.shape)} is not a dense strided tensor")
    if t.device != bucket.device:
        raise ValueError(f"{who}: tensor {i} {tuple(t.shape)} is on {t.device}, the bucket on {bucket.device}")
    if t.numel() >= 1 << 31:
        raise ValueError(f"{who}: tensor {i} {tuple(t.shape)} has {t.numel()} elements (below 2^31 expected)")


def _check_slots(offsets, sizes, bucket: torch.Tensor, who: str) -> None:
    if len(offsets) != len(sizes):
        raise ValueError(f"{who}: {len(sizes)} tensors but {len(offsets)} offsets")
    for i, (off, n) in enumerate(zip(offsets, sizes)):
        if isinstance(off, bool) or int(off) != off or off < 0 or off + n > bucket.numel():
            raise ValueError(f"{who}: slot {i} = [{off}, {off + n}) lies beyond the bucket's {bucket.numel()} elements")


def _ll_array(values):
    import ctypes as C
    return (C.c_longlong * max(len(values), 1))(*[int(v) for v in values])


def pack_grads(tensors, offsets, bucket: torch.Tensor, scale: float = 1.0, sizes=None) -> int:
    """``bucket[offsets[i] : offsets[i] + n_i] = tensors[i].reshape(-1) * scale`` for the whole list in ONE launch per ``GRADSYNC_TABLE``
    tensors, on the current stream of the bucket's device; bit for bit ``bucket[off:off+n].copy_(g).mul_(scale)``.  A ``None`` entry
    (its length taken from ``sizes[i]``) writes zeros to its slot; bucket words outside the slots are left alone.  fp32 CUDA tensors only;
    a non-contiguous tensor is made contiguous first.  Nothing synchronises.  -> the number of launches."""
    import ctypes as C
    who = "pack_grads"
    _check_bucket(bucket, who)
    tensors = list(tensors)
    if isinstance(scale, (bool, torch.Tensor)) or not isinstance(scale, (int, float)):
        raise TypeError(f"{who}: scale {scale!r}: a Python float is expected (it travels as a kernel argument)")
    if sizes is None and any(t is None for t in tensors):
        raise ValueError(f"{who}: a None entry needs its length in `sizes`")
    srcs, ns = [], []
    for i, t in enumerate(tensors):
        if t is None:
            srcs.append(None)
            ns.append(int(sizes[i]))
            continue
        _check_member(t, i, bucket, who)
        srcs.append(t if t.is_contiguous() else t.contiguous())
        ns.append(t.numel())
        if sizes is not None and int(sizes[i]) != ns[-1]:
            raise ValueError(f"{who}: tensor {i} has {ns[-1]} elements, sizes[{i}] = {sizes[i]}")
    _check_slots(list(offsets), ns, bucket, who)
    if not srcs:
        return 0
    lib = _native.load()
    numel = _ll_array(ns)
    with torch.cuda.device(bucket.device):
        ptrs = (C.c_void_p * len(srcs))(*[None if t is None else t.data_ptr() for t in srcs])
        _native.check(lib.virnet_gradsync_pack(ptrs, numel, _ll_array(list(offsets)), len(srcs), bucket.data_ptr(), bucket.numel(), float(scale),
                                               torch.cuda.current_stream(bucket.device).cuda_stream), "gradsync_pack")
    return int(lib.virnet_gradsync_launches(numel, len(srcs)))


def unpack_grads(bucket: torch.Tensor, offsets, outs, scale=1.0) -> int:
    """``outs[i].reshape(-1)[:] = bucket[offsets[i] : offsets[i] + n_i] * scale`` for the whole list in one launch per ``GRADSYNC_TABLE``
    tensors, on the current stream of the bucket's device; bit for bit ``bucket[off:off+n].clone().mul_(scale)``.  ``scale``: a Python
    float, or a one-element fp32 tensor on the bucket's device that the kernel reads (no host sync).  ``outs`` are written in place (fresh
    tensors or existing gradients); a non-contiguous one is filled through a contiguous copy.  -> the number of launches."""
    import ctypes as C
    who = "unpack_grads"
    _check_bucket(bucket, who)
    outs = list(outs)
    scale_ptr, scale_f = None, 1.0
    if isinstance(scale, torch.Tensor):
        if scale.dtype != torch.float32 or scale.numel() != 1:
            raise TypeError(f"{who}: scale tensor {tuple(scale.shape)} {scale.dtype}: one float32 element is expected")
        if scale.device != bucket.device:
            raise ValueError(f"{who}: scale is on {scale.device}, the bucket on {bucket.device}")
        scale_ptr = scale.data_ptr()
    elif isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"{who}: scale {scale!r}: a Python float or a one-element float32 tensor is expected")
    else:
        scale_f = float(scale)
    dsts = []
    for i, t in enumerate(outs):
        _check_member(t, i, bucket, who)
        dsts.append(t if t.is_contiguous() else torch.empty(t.shape, dtype=t.dtype, device=t.device))
    ns = [t.numel() for t in outs]
    _check_slots(list(offsets), ns, bucket, who)
    if not outs:
        return 0
    lib = _native.load()
    numel = _ll_array(ns)
    with torch.cuda.device(bucket.device), torch.no_grad():
        ptrs = (C.c_void_p * len(dsts))(*[t.data_ptr() for t in dsts])
        _native.check(lib.virnet_gradsync_unpack(bucket.data_ptr(), bucket.numel(), _ll_array(list(offsets)), numel, ptrs, len(dsts), scale_f,
                                                 scale_ptr, torch.cuda.current_stream(bucket.device).cuda_stream), "gradsync_unpack")
        for t, d in zip(outs, dsts):
            if d is not t:
                t.copy_(d)
    return int(lib.virnet_gradsync_launches(numel, len(dsts)))


class GradientReducer:
    """Bucketed, asynchronous gradient averaging for the training step (the job DistributedDataParallel does at
    ``train_denoising_syn.py:71``, shaped for this path).

    The whole network is ONE autograd Function here, so torch's per-parameter hooks would all fire at the end of the backward and
    nothing would overlap.  Instead the backward hands every layer's gradients to ``push`` as soon as its wgrad kernels are
    queued; they are scaled by 1/world into a flat fp32 bucket and a bucket is all-reduced (``async_op=True``: RCCL runs it on its
    own stream behind the work already queued) while the remaining layers' dgrad/wgrad kernels execute.  ``finish`` waits and returns
    COPIES of the bucket slices as the gradients (a p.grad aliasing a bucket would be overwritten by the next step's push).  Buckets are laid out in the order the first backward produced the gradients.
    On the xGMI mesh the 42 MB of denoise-syn gradients are 6 buckets of <= 8 MB; RCCL chooses the algorithm per message.

    Device gradients move through csrc/gradsync.hip: the buckets are views of one allocation, a ``push`` is ONE pack launch, ``finish`` one
    unpack launch per bucket (its ``unscale`` folds the fused backward's power-of-two factor in); CPU tensors keep the torch expressions.
    A backward that does not call ``push`` (the per-conv route) is followed by :meth:`reduce_grads`; ``begin_step()`` before the backward and
    ``ensure_reduced()`` after it give exactly one averaging per step whichever route it took.
    """

    def __init__(self, params: Iterable[torch.nn.Parameter], bucket_bytes: int = 8 << 20, group=None):
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        self.bucket_bytes = int(bucket_bytes)
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self._order: List[torch.nn.Parameter] = []          # production order seen during the first step
        self._slots: Optional[Dict[int, Tuple[int, int, int]]] = None   # id(param) -> (bucket, offset, numel)
        self._buckets: List[torch.Tensor] = []
        self._flat: Optional[torch.Tensor] = None           # device buckets: views of ONE allocation, so a push is one launch
        self._base: List[int] = []                          # element offset of every bucket in it
        self._remaining: List[int] = []
        self._members: List[int] = []
        self._produced: set = set()
        self._works: list = []
        self._observing = True                              # first step: record the production order, re-lay the buckets after it
        self.consumed = False                               # this step's gradients have been averaged (begin_step() clears it)

    # -- bucket layout ------------------------------------------------------------------------------------------------
    def _build(self, device: torch.device, order_hint: Optional[List[torch.nn.Parameter]] = None) -> None:
        base = self._order if order_hint is None else order_hint
        known = {id(p) for p in base}
        order = list(base) + [p for p in self.params if id(p) not in known]       # never-produced parameters go last
        self._slots, sizes = {}, []
        cur, used = 0, 0
        for p in order:
            n = p.numel()
            if used and (used + n) * 4 > self.bucket_bytes:
                sizes.append(used)
                cur, used = cur + 1, 0
            self._slots[id(p)] = (cur, used, n)
            used += n
        sizes.append(used)
        if device.type == "cuda":
            # one allocation, every bucket at a 512-byte boundary of it: pack_grads takes slots anywhere in the flat buffer
            self._base, total = [], 0
            for n in sizes:
                self._base.append(total)
                total += -(-n // 128) * 128
            self._flat = torch.zeros(max(total, 1), dtype=torch.float32, device=device)
            self._buckets = [self._flat[a:a + n] for a, n in zip(self._base, sizes)]
        else:
            self._flat, self._base = None, []
            self._buckets = [torch.zeros(n, dtype=torch.float32, device=device) for n in sizes]
        self._members = [0] * len(sizes)
        for b, _, _ in self._slots.values():
            self._members[b] += 1

    @property
    def bucket_sizes(self) -> List[int]:
        return [int(b.numel()) for b in self._buckets]

    # -- per step -----------------------------------------------------------------------------------------------------
    def begin_step(self) -> None:
        """Call before a backward whose route is not known: afterwards :meth:`ensure_reduced` averages exactly once."""
        self.consumed = False

    def ensure_reduced(self) -> None:
        """After ``loss.backward()``: average the gradients with :meth:`reduce_grads` unless the backward fed the reducer itself."""
        if not self.consumed:
            self.reduce_grads()

    def start(self) -> None:
        self._works = []
        if self._slots is None:
            # first step: the production order is not known yet -- lay the buckets out in REVERSE registration order (the guess
            # torch's DDP makes too: the backward visits the modules roughly back to front), so step 1 already overlaps; the
            # observed order replaces it after the step
            self._build(self.params[0].device, order_hint=list(reversed(self.params)))
        self._remaining = list(self._members)
        self._produced = set()
        if self._flat is None:
            for b in self._buckets:
                b.zero_()
        # (device buckets are not cleared: every slot is written each step, by push() or with zeros by finish())

    def _all_reduce(self, b: int) -> None:
        self._works.append(dist.all_reduce(self._buckets[b], group=self.group, async_op=True))

    def push(self, grads: Dict[torch.nn.Parameter, torch.Tensor]) -> None:
        """Scale the gradients into their bucket slots ON THE CALLER'S CURRENT STREAM (the weight-gradient side stream during the
        backward) and start the all-reduce of every bucket that became complete; the collective is ordered after that stream.
        Device gradients go in with ONE pack launch per call (csrc/gradsync.hip)."""
        scale = 1.0 / self.world
        taken = [(p, g) for p, g in grads.items() if g is not None and p.requires_grad]
        if self._observing:
            self._order.extend(p for p, _ in taken)
        if self._flat is not None and taken:
            slots = [self._slots[id(p)] for p, _ in taken]
            pack_grads([g for _, g in taken], [self._base[b] + off for b, off, _ in slots], self._flat, scale)
        for p, g in taken:
            b, off, n = self._slots[id(p)]
            if self._flat is None:
                self._buckets[b][off:off + n].copy_(g.reshape(-1)).mul_(scale)
            else:
                self._produced.add(id(p))
            self._remaining[b] -= 1
            if self._remaining[b] == 0 and self.world > 1:
                self._all_reduce(b)

    def finish(self, unscale=1.0) -> Dict[torch.nn.Parameter, torch.Tensor]:
        """Wait for the collectives -> {parameter: its averaged gradient times ``unscale``} as fresh tensors.  ``unscale``: a Python float
        or a one-element fp32 device tensor (the fused backward's power-of-two factor, which never visits the host); device buckets
        come back with ONE unpack launch per bucket."""
        if self._flat is not None:
            missing = [self._slots[id(p)] for p in self.params if id(p) not in self._produced]
            if missing:                                   # parameters nobody produced this step: zeros, in one launch
                pack_grads([None] * len(missing), [self._base[b] + off for b, off, _ in missing], self._flat, 1.0, sizes=[n for _, _, n in missing])
        if self.world > 1:
            for b, left in enumerate(self._remaining):    # buckets holding parameters nobody produced this step
                if left > 0:
                    self._all_reduce(b)
                    self._remaining[b] = 0
        for w in self._works:
            w.wait()
        self._works = []
        # Copies, not bucket views: autograd's AccumulateGrad adopts what it is handed as p.grad, and a p.grad aliasing a bucket
        # is rewritten by the NEXT step's push() before `p.grad += new` runs (zero_grad(set_to_none=False) and gradient
        # accumulation would then see 2x the new gradient).
        out = {}
        if self._flat is not None:
            per_bucket: List[list] = [[] for _ in self._buckets]
            for p in self.params:
                b, off, _ = self._slots[id(p)]
                out[p] = torch.empty(p.shape, dtype=torch.float32, device=self._flat.device)
                per_bucket[b].append((off, out[p]))
            for bucket, members in zip(self._buckets, per_bucket):
                if members:
                    unpack_grads(bucket, [off for off, _ in members], [t for _, t in members], unscale)
        else:
            for p in self.params:
                b, off, n = self._slots[id(p)]
                out[p] = self._buckets[b][off:off + n].clone().view_as(p)
                if not (isinstance(unscale, float) and unscale == 1.0):
                    out[p].mul_(unscale)
        if self._observing:                               # from step 2 on: buckets in the order the backward really produced them
            self._observing = False
            self._build(self._buckets[0].device)
        self.consumed = True
        return out

    @torch.no_grad()
    def reduce_grads(self) -> None:
        """Average the ``p.grad`` a backward left behind WITHOUT feeding the reducer (the per-conv route: the SISR net, ``noise_avg``,
        ``extra_mode`` Down / Both).  Bucket by bucket: every gradient times 1/world into its slot (one pack launch), the bucket's
        ``all_reduce(async_op=True)`` started at once; then all waited for and every slot written back IN PLACE into the same ``p.grad``
        (one unpack launch per bucket).  A ``None`` gradient stays ``None``; its slot travels as zeros, so the ranks' collectives match."""
        if not self.params:
            self.consumed = True
            return
        self.start()
        scale = 1.0 / self.world
        per_bucket: List[list] = [[] for _ in self._buckets]
        for p in self.params:
            b, off, n = self._slots[id(p)]
            per_bucket[b].append((off, n, p))
        for b, members in enumerate(per_bucket):
            if self._flat is not None:
                pack_grads([p.grad for _, _, p in members], [off for off, _, _ in members], self._buckets[b], scale, sizes=[n for _, n, _ in members])
            else:
                for off, n, p in members:
                    if p.grad is not None:
                        self._buckets[b][off:off + n].copy_(p.grad.reshape(-1)).mul_(scale)
            if self.world > 1:
                self._all_reduce(b)
        for w in self._works:
            w.wait()
        self._works = []
        self._remaining = [0] * len(self._buckets)
        for b, members in enumerate(per_bucket):
            live = [(off, n, p) for off, n, p in members if p.grad is not None]
            if self._flat is not None:
                unpack_grads(self._buckets[b], [off for off, _, _ in live], [p.grad for _, _, p in live], 1.0)
            else:
                for off, n, p in live:
                    p.grad.copy_(self._buckets[b][off:off + n].view_as(p.grad))
        self.consumed = True


class DistributedTrainer(torch.nn.Module):
    """``DistributedDataParallel``-shaped wrapper for the drop-in modules: broadcasts rank 0's parameters once, then averages the
    gradients of every backward through a :class:`GradientReducer` that overlaps the collectives with the backward kernels.

        net = DistributedTrainer(VIRAttResUNet(...).cuda(rank))      # train_denoising_syn.py:71
        mu, sigma = net(x); loss.backward(); optimizer.step()
    """

    def __init__(self, module: torch.nn.Module, bucket_bytes: int = 8 << 20, group=None):
        super().__init__()
        self.module = module
        broadcast_parameters(module, src=0, group=group)
        self.reducer = GradientReducer(module.parameters(), bucket_bytes=bucket_bytes, group=group)
        module._grad_reducer = self.reducer

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)
