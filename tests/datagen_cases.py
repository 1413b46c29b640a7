"""Shared cases of the batch-synthesis tests (tests/test_datagen_gpu.py, tests/test_redzone_datagen_gpu.py): one pool, one parameter set
per patch size, and the numpy definitions' outputs for them, computed once.

The pool: 33x47, 70x45 and 64x64.  Odd widths give rows that start at every byte alignment; the 64x64 image equals the largest patch, so its
only crop touches both ends of its slab, and it sits last: a read past the crop there is a read past the buffer.  Patch sizes 20 (no
multiple of 4: the 4-byte store form), 33 (no multiple of the 32-pixel tile: two tiles a side, one of them a single row / column) and 64
(full tiles, the 16-byte store form).  Nine samples: every augmentation flag and one repeat, crops at offset 0 and at H - P / W - P."""
import functools

import numpy as np

from virnet_amd import datagen

SHAPES = [(33, 47), (70, 45), (64, 64)]
PATCHES = (20, 33, 64)
N = 9
FLAGS = [0, 1, 2, 3, 4, 5, 6, 7, 3]


@functools.lru_cache(maxsize=None)
def images(seed: int = 0):
    g = np.random.default_rng(seed)
    return tuple(g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES)


@functools.lru_cache(maxsize=None)
def params(p: int) -> datagen.BatchParams:
    fit = [i for i, (h, w) in enumerate(SHAPES) if h >= p and w >= p]
    img = [fit[k % len(fit)] for k in range(N)]
    corner = [(0, 0), (1, 1), (0, 1), (1, 0), (1, 1), (0, 0), (1, 0), (0, 1), (1, 1)]      # crop origin as a share of (H - P, W - P)
    ind_h = [corner[k][0] * (SHAPES[img[k]][0] - p) for k in range(N)]
    ind_w = [corner[k][1] * (SHAPES[img[k]][1] - p) for k in range(N)]
    g = np.random.default_rng(p)
    center_h, center_w = g.uniform(0, p, N), g.uniform(0, p, N)
    center_h[0], center_w[0] = 0.0, float(p)              # the clamped centre: past the last pixel
    center_h[1], center_w[1] = p / 2 + 0.5, 2.5           # ties between two nearest pixels
    up, down = g.uniform(0.1, 75 / 255, N) + 5 / 255, g.uniform(0.0, 0.1, N)
    niid = [1] * N
    niid[5] = 0                                            # one iid sample among them
    return datagen.BatchParams(SHAPES, p, img, ind_h, ind_w, FLAGS, niid=niid, center_h=center_h, center_w=center_w, scale=g.uniform(p / 4, p / 4 * 3, N),
                               up=up, down=down)


@functools.lru_cache(maxsize=None)
def noise(p: int) -> np.ndarray:
    return np.random.default_rng(100 + p).standard_normal((N, 3, p, p)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def expected(p: int, clip: bool = False):
    """dict of the definitions' outputs for params(p): noisy, gt, sigma (denoise), pair_a, pair_b, hr.  Read-only."""
    ims, other = list(images(0)), list(images(1))
    noisy, gt, sigma = datagen.denoise_batch_np(ims, params(p), noise(p), clip)
    pair_a, pair_b = datagen.pair_batch_np(ims, other, params(p))
    out = dict(noisy=noisy, gt=gt, sigma=sigma, pair_a=pair_a, pair_b=pair_b, hr=datagen.hr_batch_np(ims, params(p)))
    for v in out.values():
        v.setflags(write=False)
    return out


def ulps(got, want) -> np.ndarray:
    """|got - want| in fp32 ulps of want"""
    want = np.asarray(want, dtype=np.float32)
    return np.abs(np.asarray(got, dtype=np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def same_bits(got, want) -> bool:
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint32), np.asarray(want).view(np.uint32))


def kinfo_ulps(got, want) -> float:
    """The largest error of (var_x, var_y, rho) rows in fp32 ulps.  rho of an isotropic kernel is a difference of two equal products: zero
    up to fp64 rounding (1e-18 where the reference computes it), where an ulp of the value itself means nothing; such entries must be as
    small on the device (below 1e-12, far under one ulp of any variance) and are left out of the ulp count."""
    got, want = np.asarray(got), np.asarray(want, dtype=np.float32)
    tiny = np.abs(want) < 1e-12
    assert np.abs(got[tiny]).max(initial=0.0) < 1e-12
    return float(ulps(got, want)[~tiny].max())
