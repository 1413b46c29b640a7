"""Shared inputs of the tiled-restoration tests (tests/test_restore_host.py, test_restore_gpu.py, test_restore_redzone_gpu.py): the images,
their plans, random restored stacks and the host definitions' results, each computed once.

The cases reach every branch of csrc/restore.hip: a partial last tile with a three-tile overlap (37 = starts 0, 8, 16, 21 at tile 16 /
overlap 4), a 3-byte pixel stride that breaks dword alignment (uint8 HWC, odd width), planar and interleaved sources of either type, a
width that is a multiple of four and one that is not (vector and scalar stores on both sides), more than 64 tiles (two gather launches),
an image lower than the tile, and a tile wider than one workgroup's 512 columns."""
import functools

import numpy as np
import torch

from virnet_amd import restore

#        id                   H    W    C  dtype  layout tile  overlap
CASES = [("u8_hwc_37x53x3",   37,  53,  3, "u8",  "hwc", 16,   4),
         ("f32_chw_40x56x3",  40,  56,  3, "f32", "chw", 16,   4),
         ("u8_hwc_64x100x1",  64,  100, 1, "u8",  "hwc", 16,   4),
         ("f32_hwc_37x53x3",  37,  53,  3, "f32", "hwc", 16,   4),
         ("u8_chw_37x53x4",   37,  53,  4, "u8",  "chw", 16,   4),
         ("u8_hwc_6x1100x3",  6,   1100, 3, "u8", "hwc", 1024, 4)]
IDS = [c[0] for c in CASES]
ISSUE_CASES = CASES[:3]                       # the three the issue names; the rest complete the dtype x layout grid and the wide tile
BLEND_CASES = CASES[:3] + CASES[4:5]
BLEND_IDS = [c[0] for c in BLEND_CASES]
OPTIONS = [(out, layout) for out in restore.OUTS for layout in restore.LAYOUTS]


@functools.lru_cache(maxsize=None)
def image(case) -> np.ndarray:
    name, h, w, c, dtype, layout, _, _ = case
    rng = np.random.default_rng(sum(map(ord, name)))
    shape = (h, w, c) if layout == "hwc" else (c, h, w)
    a = rng.integers(0, 256, shape, dtype=np.uint8) if dtype == "u8" else rng.random(shape, dtype=np.float32) * 1.4 - np.float32(0.2)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def plan_of(case, scale: int = 1, blend: str = "linear") -> restore.TilePlan:
    _, h, w, c, _, _, tile, overlap = case
    return restore.plan(h, w, tile, overlap, scale=scale, blend=blend, channels=c)


@functools.lru_cache(maxsize=None)
def gathered(case) -> np.ndarray:
    p = plan_of(case)
    a = restore.gather_np(image(case), p, 0, p.T, layout=case[5])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def stack(case, scale: int) -> np.ndarray:
    """A random restored stack in [-0.2, 1.2] (the clip matters), with a -0 and exact 0 / 1 among the values."""
    p = plan_of(case, scale)
    rng = np.random.default_rng(1000 + scale + sum(map(ord, case[0])))
    a = rng.random((p.T, case[3], p.tho, p.two), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)
    flat = a.reshape(-1)
    flat[::97] = 0.0
    flat[1::101] = 1.0
    flat[2::103] = -0.0
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def blended(case, scale: int, blend: str, out: str, layout: str) -> np.ndarray:
    a = restore.blend_np(stack(case, scale), plan_of(case, scale, blend), out=out, layout=layout)
    a.setflags(write=False)
    return a


def same_bits(t: torch.Tensor, want: np.ndarray) -> bool:
    got = t.detach().cpu().numpy()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.float32:
        return bool(np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)))
    return bool(np.array_equal(got, want))


def forward_tiled_index(H: int, W: int, tile: int, overlap: int, scale: int = 1, multiple: int = 4) -> np.ndarray:
    """``forward_tiled``'s stitching replayed on index arrays: [H * scale, W * scale] = the number of the tile whose write survives."""
    from virnet_amd.utils.tiling import _starts
    tile = max(multiple, tile // multiple * multiple)
    th, tw = min(tile, H), min(tile, W)
    owner = np.full((H * scale, W * scale), -1, dtype=np.int64)
    k = 0
    for y in _starts(H, th, overlap):
        for x0 in _starts(W, tw, overlap):
            t = 0 if y == 0 else overlap
            b = 0 if y + th == H else overlap
            l = 0 if x0 == 0 else overlap
            r = 0 if x0 + tw == W else overlap
            owner[(y + t) * scale:(y + th - b) * scale, (x0 + l) * scale:(x0 + tw - r) * scale] = k
            k += 1
    return owner
