"""Tiled restoration of whole photographs on the device (csrc/restore.hip).

One image's activation tensor has to stay below 2 GB (``h * w * channels * 4 < 2**31``: csrc/conv_f16_common.h ``check_conv_desc``, the
entry and exit convolutions), which at 96 channels is about 5.5 million pixels: a 12 MP photograph does not go through ``net(x)``.  Here
the image stays on the device as it was read (uint8 or float32, HWC or CHW), is cut into overlapping tiles by ONE launch per chunk
(:func:`gather`), the tiles go through the ordinary forward, and ONE launch per output puts them together again (:func:`blend`), clipped
and quantised on the way out.  Only those two kernels see the whole image; every tensor the forward sees is one batch of tiles, sized by
:func:`auto_tile` to stay inside the limit.

The grid is the one of ``utils/tiling.forward_tiled`` (tile rounded down to a multiple of ``multiple``, starts by ``tiling._starts``).
A :class:`TilePlan` holds it together with two TAP TABLES, one per axis: for every output row (column) up to ``K = 3`` slots of
``(tile index along the axis, float32 weight)`` in ascending tile order, -1 for an unused slot.

  * ``blend="crop"``: one slot of weight 1 -- the LAST tile whose kept interior (the tile minus ``overlap * scale`` on every side that is
    not an image border) holds the position.  That is what ``forward_tiled`` computes, bit for bit: it writes the interiors in tile order
    and later tiles overwrite earlier ones.
  * ``blend="linear"``: tile ``i`` (input pixels ``[s, s + t)``) has the raw weight ``min(L, R, 2 * overlap * scale)`` at output position
    ``q`` with ``L = q - s * scale + 1`` unless the tile starts at the image border and ``R = (s + t) * scale - q`` unless it ends there;
    the weights of the covering tiles are normalised in float64 and rounded once to float32.  A position under one tile has weight 1.0.

The definitions are :func:`gather_np` and :func:`blend_np`; the kernels give the same bits:

  * uint8 sources become ``np.float32(u / 255.0)`` (as ``ensemble.expand``), float32 sources pass through;
  * the blended value is ``acc = 0; acc = fl(acc + fl(fl(wy * wx) * v))`` over the used row slots and, inside them, the used column slots,
    in ascending order, in float32 without contraction.  Unused slots are skipped, so a NaN (the range guard's poison) stays inside the
    support of the tile that holds it.  In crop mode the value is copied;
  * ``out="uint8"`` is ``eval.img_as_ubyte(clip(.))`` (the arithmetic of ``metrics.to_uint8``), ``out="float32"`` is ``np.clip(., 0, 1)`` or,
    with ``clip=False``, the raw value.

Nothing here synchronises; both kernels can be captured (build the plan's device tables first: ``plan.tables(device)``), are bitwise
reproducible and do not depend on how the tiles are cut into chunks.  CPU tensors raise (no fallback).
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _native
from . import eval as veval
from .utils import tiling

K = _native.TILE_SLOTS
MAX_BOXES = _native.TILE_BOXES
MAX_CHANNELS = 4
MAX_AUTO_TILE = 1024
LIMIT_BYTES = 2 ** 31       # csrc/conv_f16_common.h check_conv_desc, virnet_conv_entry, virnet_conv_exit
MAX_ELEMENTS = 2 ** 31
BLENDS = ("linear", "crop")
OUTS = ("uint8", "float32")
LAYOUTS = ("hwc", "chw")


# ---- the one-pass limit ------------------------------------------------------------------------------------------------------------------
def fits(h: int, w: int, channels: int, limit_bytes: int = LIMIT_BYTES) -> bool:
    """The library's bound on one image's activation tensor: ``h * w * channels * 4 < limit_bytes`` with the channel count as the
    library pads it (``check_conv_desc``: n_pad / cin_pad)."""
    return int(h) * int(w) * int(channels) * 4 < int(limit_bytes)


def _pad(c: int, m: int) -> int:
    return -(-int(c) // m) * m


def widest_channels(net) -> int:
    """Channels per full-resolution pixel of the widest activation a forward of ``net`` makes, padded as the library pads them (output
    channels to 32): level ``l`` of the U-Net holds ``n_feat[l]`` channels on a grid ``4**l`` times smaller, SNet its filters."""
    widths = [-(-_pad(nf, 32) // 4 ** lvl) for lvl, nf in enumerate(net.RNet.n_feat)]
    widths.append(_pad(net.SNet.conv1.weight.shape[0], 32))                 # (KNet's head has stride 4: 1/16 of the pixels)
    return max(widths)


def auto_tile(H: int, W: int, widest: int, scale: int = 1, limit_bytes: int = LIMIT_BYTES, multiple: int = 4) -> int:
    """The largest tile (a multiple of ``multiple``, at most 1024) whose widest activation ``th*scale x tw*scale x widest`` passes
    :func:`fits`; 0 when the whole image does (one pass)."""
    H, W, scale, multiple = int(H), int(W), int(scale), int(multiple)
    if fits(H * scale, W * scale, widest, limit_bytes):
        return 0
    tile = MAX_AUTO_TILE // multiple * multiple
    while tile >= multiple:
        if fits(min(tile, H) * scale, min(tile, W) * scale, widest, limit_bytes):
            return tile
        tile -= multiple
    raise ValueError(f"no tile of at least {multiple} pixels keeps {widest} channels at scale {scale} below {limit_bytes} bytes")


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def _axis_taps(size: int, t: int, starts: Sequence[int], overlap: int, scale: int, blend: str) -> Tuple[np.ndarray, np.ndarray]:
    """(idx int32 [size * scale, K], weight float32 [size * scale, K]) of one axis."""
    n_out = size * scale
    q = np.arange(n_out, dtype=np.int64)
    idx = np.full((n_out, K), -1, dtype=np.int32)
    wgt = np.zeros((n_out, K), dtype=np.float64)
    if blend == "crop":
        for i, s in enumerate(starts):                     # ascending: later tiles overwrite, as forward_tiled's writes do
            lo = (s + (0 if s == 0 else overlap)) * scale
            hi = (s + t - (0 if s + t == size else overlap)) * scale
            idx[lo:hi, 0] = i
        if (idx[:, 0] < 0).any():
            raise AssertionError("crop plan leaves a position without an owner")
        wgt[:, 0] = 1.0
        return idx, wgt.astype(np.float32)
    cap = 2 * overlap * scale
    raw = np.zeros((len(starts), n_out), dtype=np.float64)
    for i, s in enumerate(starts):
        lo, hi = s * scale, (s + t) * scale
        r = np.full(n_out, cap, dtype=np.int64)
        if s != 0:
            r = np.minimum(r, q - lo + 1)
        if s + t != size:
            r = np.minimum(r, hi - q)
        raw[i, lo:hi] = r[lo:hi]
    count = (raw > 0).sum(axis=0)
    if count.max() > K:
        at = int(np.argmax(count))
        raise ValueError(f"output position {at} lies under {int(count.max())} tiles, at most {K} can be blended: use a larger tile or a smaller "
                         f"overlap (tile {t}, overlap {overlap}: the tile should be at least four times the overlap)")
    if count.min() < 1:
        raise AssertionError("linear plan leaves a position without a tile")
    total = raw.sum(axis=0)
    fill = np.zeros(n_out, dtype=np.int64)
    for i in range(len(starts)):
        on = raw[i] > 0
        idx[on, fill[on]] = i
        wgt[on, fill[on]] = raw[i, on] / total[on]
        fill[on] += 1
    return idx, wgt.astype(np.float32)


class TilePlan:
    """The tile grid of an ``H x W`` image and its tap tables (see the module docstring).  ``boxes``: the ``(y, x)`` origins in the order
    ``forward_tiled`` visits them (tile ``iy * nx + ix``); ``th, tw``: the tile in input pixels; ``row_idx / row_w``, ``col_idx / col_w``:
    the tables, ``[H * scale, K]`` and ``[W * scale, K]``."""

    def __init__(self, H: int, W: int, tile: int, overlap: int, scale: int = 1, multiple: int = 4, blend: str = "linear",
                 channels: int = 3):
        for name, v in (("H", H), ("W", W), ("tile", tile), ("scale", scale), ("multiple", multiple), ("channels", channels)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError(f"{name} {v!r}: a positive integer expected")
        if isinstance(overlap, bool) or int(overlap) != overlap or int(overlap) < 0:
            raise ValueError(f"overlap {overlap!r}: a non-negative integer expected")
        if blend not in BLENDS:
            raise ValueError(f"blend {blend!r}: expected one of {BLENDS}")
        if int(channels) > MAX_CHANNELS:
            raise ValueError(f"{channels} channels: at most {MAX_CHANNELS}")
        self.H, self.W, self.overlap, self.scale, self.multiple, self.blend = int(H), int(W), int(overlap), int(scale), int(multiple), blend
        self.channels = int(channels)
        self.tile = max(self.multiple, int(tile) // self.multiple * self.multiple)           # forward_tiled's rounding
        self.th, self.tw = min(self.tile, self.H), min(self.tile, self.W)
        if blend == "linear" and self.overlap < 1 and (self.H > self.th or self.W > self.tw):
            raise ValueError("blend='linear' needs an overlap of at least 1 (overlap 0 leaves nothing to blend: use blend='crop')")
        self.ys, self.xs = tiling._starts(self.H, self.th, self.overlap), tiling._starts(self.W, self.tw, self.overlap)
        self.ny, self.nx = len(self.ys), len(self.xs)
        self.boxes: List[Tuple[int, int]] = [(y, x) for y in self.ys for x in self.xs]
        self.T = len(self.boxes)
        self.Ho, self.Wo, self.tho, self.two = self.H * self.scale, self.W * self.scale, self.th * self.scale, self.tw * self.scale
        if self.H * self.W * self.channels >= MAX_ELEMENTS or self.Ho * self.Wo * self.channels >= MAX_ELEMENTS:
            raise ValueError(f"an image of {self.H}x{self.W}x{self.channels} at scale {self.scale} reaches 2^31 elements: restore it in bands")
        if self.stack_elements(self.channels) >= MAX_ELEMENTS:
            raise ValueError(f"the stack of {self.T} restored tiles of {self.channels}x{self.tho}x{self.two} reaches 2^31 elements "
                             f"({self.stack_elements(self.channels)}): use a smaller image band or a larger tile")
        step = self.tile - 2 * self.overlap
        for starts, size, t in ((self.ys, self.H, self.th), (self.xs, self.W, self.tw)):       # the kernel's rule for a tile's start
            assert all(s == min(i * step, size - t) for i, s in enumerate(starts)), (starts, size, t)
        self.step_y = step if self.ny > 1 else 0
        self.step_x = step if self.nx > 1 else 0
        self.row_idx, self.row_w = _axis_taps(self.H, self.th, self.ys, self.overlap, self.scale, blend)
        self.col_idx, self.col_w = _axis_taps(self.W, self.tw, self.xs, self.overlap, self.scale, blend)
        self._tables = {}

    def stack_elements(self, channels: int) -> int:
        return self.T * int(channels) * self.tho * self.two

    def resident_bytes(self, image_itemsize: int = 1, outputs: Sequence[int] = (3,), out_itemsize: int = 1, batch: int = 8) -> int:
        """Bytes a run keeps on the device besides the forward's own workspaces: the image, one chunk of input tiles, one restored stack
        per output (``outputs``: their channel counts), the blended results and the tap tables."""
        image = self.H * self.W * self.channels * int(image_itemsize)
        chunk = min(int(batch), self.T) * self.channels * self.th * self.tw * 4
        stacks = sum(self.stack_elements(c) * 4 for c in outputs)
        results = sum(self.Ho * self.Wo * c * int(out_itemsize) for c in outputs)
        return image + chunk + stacks + results + self.table_blob().nbytes

    def table_blob(self) -> np.ndarray:
        """The four tables as the kernel reads them, one int32 array: row_idx, row_w, col_idx, col_w, each ``[K][pitch]`` (slot-major,
        pitch = the axis length rounded up to four; the float weights as their bit patterns)."""
        parts = []
        for idx, wgt in ((self.row_idx, self.row_w), (self.col_idx, self.col_w)):
            pitch = _pad(idx.shape[0], 4)
            i = np.full((K, pitch), -1, dtype=np.int32)
            w = np.zeros((K, pitch), dtype=np.float32)
            i[:, :idx.shape[0]] = idx.T
            w[:, :idx.shape[0]] = wgt.T
            parts += [i.reshape(-1), w.view(np.int32).reshape(-1)]
        return np.concatenate(parts)

    def tables(self, device) -> Tensor:
        """The blob on ``device``: built once per device, uploaded in one pinned copy (do this before a graph capture)."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"tables on {dev}: the VIRNet HIP path runs on a ROCm device only (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        t = self._tables.get(dev)
        if t is None:
            with _native.capture_lock:
                t = self._tables[dev] = torch.from_numpy(self.table_blob()).pin_memory().to(dev, non_blocking=True)
        return t

    def adopt_tables(self, t: Tensor) -> None:
        """Use ``t`` (a device copy of :meth:`table_blob` in memory of the caller's choosing) as the tables of its device."""
        if t.dtype != torch.int32 or t.numel() != self.table_blob().size or not t.is_cuda or not t.is_contiguous():
            raise ValueError("adopt_tables takes a contiguous int32 CUDA copy of table_blob()")
        self._tables[t.device] = t

    def __repr__(self) -> str:
        return (f"TilePlan({self.H}x{self.W}, tile {self.th}x{self.tw}, overlap {self.overlap}, scale {self.scale}, {self.blend}: "
                f"{self.ny}x{self.nx} tiles)")


def plan(H: int, W: int, tile: int, overlap: int, scale: int = 1, multiple: int = 4, blend: str = "linear", channels: int = 3) -> TilePlan:
    """The :class:`TilePlan` of an ``H x W`` image (host only, no device).  Raises when ``tile <= 2 * overlap``, when a position would lie
    under more than three tiles, and when the image or a restored stack of ``channels`` channels reaches 2^31 elements."""
    return TilePlan(H, W, tile, overlap, scale, multiple, blend, channels)


# ---- definitions on the host -------------------------------------------------------------------------------------------------------------
def _image_shape(shape, layout: str) -> Tuple[int, int, int]:
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: expected one of {LAYOUTS}")
    if len(shape) == 2:
        return int(shape[0]), int(shape[1]), 1
    if len(shape) != 3:
        raise ValueError(f"image must be [H,W,C], [C,H,W] or [H,W], got {tuple(shape)}")
    h, w, c = (int(s) for s in (shape if layout == "hwc" else (shape[1], shape[2], shape[0])))
    if c < 1 or c > MAX_CHANNELS:
        raise ValueError(f"image has {c} channels, 1..{MAX_CHANNELS} expected")
    return h, w, c


def _check_image(shape, layout: str, p: TilePlan) -> Tuple[int, int, int]:
    h, w, c = _image_shape(shape, layout)
    if (h, w) != (p.H, p.W):
        raise ValueError(f"image is {h}x{w}, the plan was made for {p.H}x{p.W}")
    return h, w, c


def _check_range(p: TilePlan, first: int, last: int) -> Tuple[int, int]:
    first, last = int(first), int(last)
    if not 0 <= first < last <= p.T:
        raise ValueError(f"tiles {first}..{last}: the plan has {p.T} tiles (first < last expected)")
    return first, last


def gather_np(image: np.ndarray, p: TilePlan, first: int, last: int, layout: str = "hwc") -> np.ndarray:
    """Tiles ``first .. last - 1`` of ``image`` (uint8 or float32) as a float32 ``[n,C,th,tw]`` array."""
    image = np.asarray(image)
    if image.dtype not in (np.uint8, np.float32):
        raise TypeError(f"image must be uint8 or float32, got {image.dtype}")
    _, _, c = _check_image(image.shape, layout, p)
    first, last = _check_range(p, first, last)
    chw = image.reshape(c, p.H, p.W) if layout == "chw" or image.ndim == 2 else image.transpose(2, 0, 1)
    unit = (chw / 255.0).astype(np.float32) if image.dtype == np.uint8 else chw
    return np.stack([np.ascontiguousarray(unit[:, y:y + p.th, x:x + p.tw]) for y, x in p.boxes[first:last]])


def _finish_np(chw: np.ndarray, out: str, layout: str, clip: bool) -> np.ndarray:
    if out == "uint8":
        res = veval.img_as_ubyte(chw.clip(0, 1))
    else:
        res = np.clip(chw, np.float32(0), np.float32(1)) if clip else chw
    return np.ascontiguousarray(res.transpose(1, 2, 0)) if layout == "hwc" else np.ascontiguousarray(res)


def _options(out: str, layout: str) -> None:
    if out not in OUTS:
        raise ValueError(f"out {out!r}: expected one of {OUTS}")
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: expected one of {LAYOUTS}")


def _check_stack(shape, p: TilePlan) -> int:
    if len(shape) != 4 or tuple(int(s) for s in shape[2:]) != (p.tho, p.two) or int(shape[0]) != p.T:
        raise ValueError(f"tiles must be [{p.T},C,{p.tho},{p.two}], got {tuple(shape)}")
    c = int(shape[1])
    if c < 1 or c > MAX_CHANNELS:
        raise ValueError(f"tiles have {c} channels, 1..{MAX_CHANNELS} expected")
    if p.stack_elements(c) >= MAX_ELEMENTS or p.Ho * p.Wo * c >= MAX_ELEMENTS:
        raise ValueError(f"a stack of {p.T} tiles of {c}x{p.tho}x{p.two} (or its {p.Ho}x{p.Wo} image) reaches 2^31 elements: use a smaller "
                         f"image band or a larger tile")
    return c


def blend_np(tiles: np.ndarray, p: TilePlan, out: str = "uint8", layout: str = "hwc", clip: bool = True) -> np.ndarray:
    """The restored stack ``[T,C,th*scale,tw*scale]`` (float32) as one image."""
    _options(out, layout)
    tiles = np.asarray(tiles)
    if tiles.dtype != np.float32:
        raise TypeError(f"tiles must be float32, got {tiles.dtype}")
    c = _check_stack(tiles.shape, p)
    qy, qx = np.arange(p.Ho)[:, None], np.arange(p.Wo)[None, :]
    ch = np.arange(c)[:, None, None]
    ys, xs = np.asarray(p.ys) * p.scale, np.asarray(p.xs) * p.scale

    def value(sy: int, sx: int):
        iy, ix = p.row_idx[:, sy][:, None], p.col_idx[:, sx][None, :]
        used = np.broadcast_to((iy >= 0) & (ix >= 0), (p.Ho, p.Wo))
        iy0, ix0 = np.maximum(iy, 0), np.maximum(ix, 0)
        ly, lx = np.clip(qy - ys[iy0], 0, p.tho - 1), np.clip(qx - xs[ix0], 0, p.two - 1)
        return used, tiles[(iy0 * p.nx + ix0)[None], ch, ly[None], lx[None]]

    if p.blend == "crop":
        _, acc = value(0, 0)
    else:
        acc = np.zeros((c, p.Ho, p.Wo), dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for sy in range(K):
                for sx in range(K):
                    used, v = value(sy, sx)
                    w = p.row_w[:, sy][:, None] * p.col_w[:, sx][None, :]                   # float32 product, rounded once
                    acc = np.where(used[None], acc + w[None] * v, acc)
        assert acc.dtype == np.float32
    return _finish_np(np.ascontiguousarray(acc), out, layout, clip)


# ---- the device path ---------------------------------------------------------------------------------------------------------------------
_NO_DEVICE = "the VIRNet HIP path runs on a ROCm device only (no CPU fallback)"


def _device_image(image, layout: str) -> Tensor:
    if isinstance(image, np.ndarray):
        if image.dtype not in (np.uint8, np.float32):
            raise TypeError(f"image must be uint8 or float32, got {image.dtype}")
        _image_shape(image.shape, layout)
        if not torch.cuda.is_available():
            raise RuntimeError(f"no ROCm device: {_NO_DEVICE}")
        host = np.ascontiguousarray(image) if image.flags.writeable else np.array(image)          # (torch refuses read-only memory)
        return torch.from_numpy(host).to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
    if not isinstance(image, Tensor):
        raise TypeError(f"image must be a numpy array or a CUDA tensor, got {type(image).__name__}")
    if image.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"image must be uint8 or float32, got {image.dtype}")
    _image_shape(image.shape, layout)
    if not image.is_cuda:
        raise RuntimeError(f"image is on {image.device}: {_NO_DEVICE}")
    return image.detach().contiguous()


def _gather_into(src: Tensor, p: TilePlan, first: int, last: int, layout: str, c: int, dst: Tensor) -> None:
    lib = _native.load()
    for a in range(first, last, MAX_BOXES):
        b = min(a + MAX_BOXES, last)
        flat = [v for box in p.boxes[a:b] for v in box]
        boxes = (C.c_int * len(flat))(*flat)
        _native.check(lib.virnet_tile_gather(src.data_ptr(), int(src.dtype == torch.float32), int(layout == "chw" or src.dim() == 2), p.H, p.W, c,
                                             boxes, b - a, p.th, p.tw, dst[a - first:].data_ptr(), _native.stream_handle()), "tile_gather")


def gather(image, p: TilePlan, first: int, last: int, layout: str = "hwc") -> Tensor:
    """Tiles ``first .. last - 1`` of the plan as one float32 ``[n,C,th,tw]`` batch, one launch per 64 tiles.  ``image``: uint8 or float32,
    ``[H,W,C]`` (``layout="hwc"``), ``[C,H,W]`` (``"chw"``) or ``[H,W]``, C up to 4; a CUDA tensor, or a numpy array (uploaded once)."""
    src = _device_image(image, layout)
    _, _, c = _check_image(src.shape, layout, p)
    first, last = _check_range(p, first, last)
    with torch.cuda.device(src.device):
        dst = torch.empty((last - first, c, p.th, p.tw), dtype=torch.float32, device=src.device)
        _gather_into(src, p, first, last, layout, c, dst)
    return dst


def blend(tiles: Tensor, p: TilePlan, out: str = "uint8", layout: str = "hwc", clip: bool = True) -> Tensor:
    """The restored stack ``[T,C,th*scale,tw*scale]`` as one image in one launch: ``[H*scale,W*scale,C]`` or ``[C,H*scale,W*scale]``, uint8
    (clipped and quantised) or float32 (clipped unless ``clip=False``)."""
    _options(out, layout)
    if not isinstance(tiles, Tensor):
        raise TypeError(f"tiles must be a CUDA tensor, got {type(tiles).__name__}")
    if tiles.dtype != torch.float32:
        raise TypeError(f"tiles must be float32, got {tiles.dtype}")
    c = _check_stack(tiles.shape, p)
    if not tiles.is_cuda:
        raise RuntimeError(f"tiles is on {tiles.device}: {_NO_DEVICE}")
    tiles = tiles.detach().contiguous()
    with torch.cuda.device(tiles.device):
        tab = p.tables(tiles.device)
        rp, cp = _pad(p.Ho, 4), _pad(p.Wo, 4)
        base, sec = tab.data_ptr(), 4 * K
        res = torch.empty((p.Ho, p.Wo, c) if layout == "hwc" else (c, p.Ho, p.Wo), dtype=torch.uint8 if out == "uint8" else torch.float32,
                          device=tiles.device)
        _native.check(_native.load().virnet_tile_blend(
            tiles.data_ptr(), base, base + sec * rp, base + 2 * sec * rp, base + 2 * sec * rp + sec * cp, rp, cp, p.ny, p.nx, c, p.tho, p.two,
            p.step_y * p.scale, p.Ho - p.tho, p.step_x * p.scale, p.Wo - p.two, p.Ho, p.Wo, res.data_ptr(), int(out == "float32"),
            int(layout == "chw"), int(bool(clip)), int(p.blend == "crop"), _native.stream_handle()), "tile_blend")
    return res


_blend = blend            # (restore_image has a parameter of that name)


def restore_tiles(forward: Callable, image, p: TilePlan, batch: int = 8, layout: str = "hwc") -> Union[Tensor, Tuple[Tensor, ...]]:
    """Any ``forward: [n,C,th,tw] -> tensor or tuple of tensors [n,C',th*scale,tw*scale]`` over the plan's tiles in chunks of at most
    ``batch`` (the chunks of ``forward_tiled``): one resident float32 stack ``[T,C',th*scale,tw*scale]`` per output."""
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"batch {batch}: at least 1")
    src = _device_image(image, layout)
    _, _, c = _check_image(src.shape, layout, p)
    stacks: Optional[List[Tensor]] = None
    single = False
    with torch.cuda.device(src.device):
        for a in range(0, p.T, batch):
            b = min(a + batch, p.T)
            x = torch.empty((b - a, c, p.th, p.tw), dtype=torch.float32, device=src.device)
            _gather_into(src, p, a, b, layout, c, x)
            res = forward(x)
            single = isinstance(res, Tensor)
            outs = (res,) if single else tuple(res)
            for o in outs:
                if not isinstance(o, Tensor) or not o.is_cuda or o.dtype != torch.float32 or o.dim() != 4 or \
                        (o.shape[0], o.shape[2], o.shape[3]) != (b - a, p.tho, p.two):
                    raise ValueError(f"forward must map a float32 CUDA tensor {tuple(x.shape)} to [{b - a},C',{p.tho},{p.two}] float32 tensors, got "
                                     f"{tuple(getattr(o, 'shape', ()))} {getattr(o, 'dtype', type(o).__name__)}")
            if stacks is None:
                for o in outs:
                    _check_stack((p.T, o.shape[1], p.tho, p.two), p)
                if (a, b) == (0, p.T):
                    return res if single else outs
                stacks = [torch.empty((p.T, o.shape[1], p.tho, p.two), dtype=torch.float32, device=src.device) for o in outs]
            for s, o in zip(stacks, outs):
                s[a:b].copy_(o)
    return stacks[0] if single else tuple(stacks)


def _quantise(x: Tensor, out: str, layout: str, clip: bool = True) -> Tensor:
    """One restored image ``[1,C,H,W]`` through the blend kernel's exit alone (a plan of one tile)."""
    _, c, h, w = x.shape
    p = TilePlan(h, w, max(h, w), 0, blend="crop", multiple=1, channels=c)
    return blend(x, p, out=out, layout=layout, clip=clip)


def restore_image(net, image, sf: Optional[int] = None, tile: Union[int, str] = "auto", overlap: int = 32, blend: str = "linear",
                  out: str = "uint8", layout: str = "hwc", batch: int = 8, sigma: bool = False, image_layout: str = "hwc",
                  limit_bytes: int = LIMIT_BYTES, clip: bool = True):
    """A photograph of any size through ``net`` on the device: uint8 or float32 in (``[H,W,C]``, or ``[C,H,W]`` with
    ``image_layout="chw"``), uint8 or float32 out, nothing visits the host.

    ``VIRAttResUNet``: the whole forward is tiled; returns ``mu``, or ``(mu, sigma_map)`` with ``sigma=True`` (the variance map always
    float32, un-clipped, in ``layout``).  ``VIRAttResUNetSR`` (``sf`` required): SNet and KNet run ONCE on the whole low-resolution image
    and only RNet is tiled, as ``tiling.forward_tiled_sisr`` does; returns ``(mu, kinfo, sigma)``.  The whole run is ONE range-guarded
    forward (``engine._range_guarded``): an fp16 overflow in any tile repeats the image in fp32 once.

    ``tile="auto"``: :func:`auto_tile` for the network's widest activation; when the image fits one pass the call is the plain forward
    followed by the quantisation.  ``tile=0`` forces that.  ``blend``: ``"linear"`` (ramps across the overlaps) or ``"crop"``
    (``forward_tiled``'s hard seams, bit for bit).  ``clip=False`` (float32 output only) leaves ``mu`` as the network gave it;
    ``limit_bytes`` is the bound ``tile="auto"`` sizes the tiles for (the library's 2 GB unless a test wants tiles on a small image)."""
    from . import engine
    from .networks import VIRAttResUNet, VIRAttResUNetSR
    _options(out, layout)
    if blend not in BLENDS:
        raise ValueError(f"blend {blend!r}: expected one of {BLENDS}")
    sisr = isinstance(net, VIRAttResUNetSR)
    if not sisr and not isinstance(net, VIRAttResUNet):
        raise TypeError(f"restore_image takes a VIRAttResUNet or a VIRAttResUNetSR, got {type(net).__name__}")
    if sisr:
        if sf is None or int(sf) != sf or int(sf) < 1:
            raise ValueError(f"sf {sf!r}: VIRAttResUNetSR needs a positive integer scale factor")
        if not net.noise_avg:
            raise ValueError("restore_image tiles RNet under a global conditioning: VIRAttResUNetSR with noise_avg=True expected")
    elif net.SNet.noise_avg:
        raise ValueError("a noise_avg=True denoiser pools SNet over its input: tiles would each get their own estimate")
    scale = int(sf) if sisr else 1
    src = _device_image(image, image_layout)
    h, w, c = _image_shape(src.shape, image_layout)
    if c != net.SNet.in_channels:
        raise ValueError(f"image has {c} channels, the network was built for {net.SNet.in_channels}")
    multiple = 1 << (net.RNet.depth - 1)
    widest = widest_channels(net)
    if isinstance(tile, str):
        if tile != "auto":
            raise ValueError(f"tile {tile!r}: 'auto', 0 or a tile size expected")
        tile = auto_tile(h, w, widest, scale, limit_bytes, multiple)
    tile = int(tile)
    if sisr and not fits(h, w, widest, limit_bytes):
        raise ValueError(f"the low-resolution image {h}x{w} is itself too large for SNet / KNet in one pass ({widest} channels reach "
                         f"{limit_bytes} bytes): tiling covers RNet only")
    rounded = max(multiple, tile // multiple * multiple)                     # (forward_tiled's rule for "the image fits one tile")
    p = None if tile == 0 or (h <= rounded and w <= rounded) else TilePlan(h, w, tile, overlap, scale, multiple, blend, c)
    if p is not None:
        p.tables(src.device)

    with torch.no_grad(), torch.cuda.device(src.device):
        whole = TilePlan(h, w, max(h, w), 0, blend="crop", multiple=1, channels=c)

        def full() -> Tensor:                                # the image as the modules take it: [1,C,h,w] float32
            x = torch.empty((1, c, h, w), dtype=torch.float32, device=src.device)
            _gather_into(src, whole, 0, 1, image_layout, c, x)
            return x

        if sisr:
            def run():
                x = full()
                sig, kinfo, rnet = tiling._sisr_conditioning(net, x, scale)
                if p is None:
                    return rnet(x), kinfo, sig
                return restore_tiles(rnet, src, p, batch, image_layout), kinfo, sig
        elif p is None:
            def run():
                return engine._denoise_forward(net, full())
        else:
            def run():
                return restore_tiles(lambda t: engine._denoise_forward(net, t), src, p, batch, image_layout)

        res = engine._range_guarded(run, src)
        if engine.guard_check_mode() == "deferred":
            engine.guard_poll()                              # (the stacks must be final before they are blended)
        finish = _quantise if p is None else (lambda t, **kw: _blend(t, p, **kw))
        mu = finish(res[0], out=out, layout=layout, clip=clip)
        if sisr:
            return mu, res[1], res[2]
        if not sigma:
            return mu
        return mu, finish(res[1], out="float32", layout=layout, clip=False)
