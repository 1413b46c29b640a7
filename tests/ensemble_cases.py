"""Seeded inputs of the self-ensemble tests (test_ensemble_host.py, test_ensemble_gpu.py, test_redzone_ensemble_gpu.py) and the host
definitions' results for them, computed once and shared read-only.

Shapes: one pixel, a partial tile, an exact tile, one past a tile in one direction and one short in the other, non-square over several
tiles; C 1 and 3; B 1 and 3.  The uint8 sources run through all 256 byte values.  The restored-orientation inputs of ``reduce`` are built
per OUTPUT pixel as an octet (the eight values that meet in it) and then carried to where each orientation holds them; the octets mix
  * uniform values in [0,1) (sequential and pairwise sums differ for about 38 % of them),
  * values below 0 and above 1, octets entirely below 0 / above 1,
  * zeros of either sign (all -0, all +0, mixed),
  * eight equal values at a tie (k + 0.5) / 255 as float32 and one ulp to either side of it (the sum and the division are exact),
  * eight byte-grid values float32(u / 255) whose bytes add up to 8 k + 4: a mean within rounding of the tie (k + 0.5) / 255.
"""
import functools
import itertools

import numpy as np

from virnet_amd import ensemble
from virnet_amd import eval as veval

SHAPES = [(1, 1), (5, 3), (32, 32), (33, 31), (36, 52), (64, 96)]
CASES = [(h, w, c, b) for (h, w), c, b in itertools.product(SHAPES, (1, 3), (1, 3))]
IDS = [f"{h}x{w}-c{c}-b{b}" for h, w, c, b in CASES]
EDGE_CASES = [k for k in CASES if k[:2] in ((5, 3), (33, 31), (36, 52))]          # partial tiles and non-square (red-zone file)
EDGE_IDS = [IDS[CASES.index(k)] for k in EDGE_CASES]
OPTIONS = list(itertools.product(ensemble.ORDERS, ensemble.OUTS, ensemble.LAYOUTS))
OPTION_IDS = ["-".join(o) for o in OPTIONS]


def _seed(case, salt):
    h, w, c, b = case
    return [salt, h, w, c, b]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def source_u8(case):
    """uint8 [B,H,W,C]: a seeded permutation of the byte values repeated over the elements (every value once per 256 elements)."""
    h, w, c, b = case
    n = b * h * w * c
    rng = np.random.default_rng(_seed(case, 1))
    vals = np.concatenate([rng.permutation(256) for _ in range(-(-n // 256))])[:n]
    return _frozen(vals.astype(np.uint8).reshape(b, h, w, c))


@functools.lru_cache(maxsize=None)
def source_f32(case):
    """float32 [B,H,W,C] with values outside [0,1], zeros of both signs and a denormal: they must pass bit for bit."""
    h, w, c, b = case
    rng = np.random.default_rng(_seed(case, 2))
    a = rng.uniform(-0.25, 1.25, size=(b, h, w, c)).astype(np.float32)
    flat = a.reshape(-1)
    flat[::7] = np.float32(-0.0)
    flat[3::11] = np.float32(1e-42)
    return _frozen(a)


@functools.lru_cache(maxsize=None)
def octets(case):
    """float32 [B,H,W,C,8]: the eight restored values that meet in every output element."""
    h, w, c, b = case
    n = b * h * w * c
    rng = np.random.default_rng(_seed(case, 3))
    o = rng.random((n, 8), dtype=np.float32)
    kind = rng.permutation(n) % 8                                   # 0..2: the uniform octets stay
    k = kind == 3
    o[k] = rng.uniform(-0.5, 1.5, size=(int(k.sum()), 8)).astype(np.float32)
    k = np.flatnonzero(kind == 4)                                   # eight equal values at / next to a tie
    tie = ((rng.integers(0, 255, size=len(k)) + 0.5) / 255.0).astype(np.float32)
    side = rng.integers(-1, 2, size=len(k))
    tie = np.where(side < 0, np.nextafter(tie, np.float32(0)), np.where(side > 0, np.nextafter(tie, np.float32(1)), tie))
    o[k] = tie[:, None]
    k = np.flatnonzero(kind == 5)                                   # zeros: all -0, all +0, mixed signs
    which = rng.integers(0, 3, size=len(k))
    signs = np.where(rng.integers(0, 2, size=(len(k), 8)) == 1, np.float32(-0.0), np.float32(0.0))
    o[k] = np.where((which == 0)[:, None], np.float32(-0.0), np.where((which == 1)[:, None], np.float32(0.0), signs))
    k = np.flatnonzero(kind == 6)                                   # entirely below 0 / above 1
    lo = rng.uniform(-1.0, -1e-3, size=(len(k), 8)).astype(np.float32)
    hi = rng.uniform(1.0 + 1e-3, 2.0, size=(len(k), 8)).astype(np.float32)
    o[k] = np.where((rng.integers(0, 2, size=len(k)) == 1)[:, None], lo, hi)
    k = np.flatnonzero(kind == 7)                                   # byte-grid values whose bytes add up to 8 j + 4
    u = rng.integers(4, 248, size=(len(k), 8))
    u[:, 7] += (4 - u.sum(axis=1)) % 8
    o[k] = (u / 255.0).astype(np.float32)
    return _frozen(o.reshape(b, h, w, c, 8))


@functools.lru_cache(maxsize=None)
def restored(case):
    """(even [4B,C,H,W], odd [4B,C,W,H]) float32: orientation m of image b holds ``dihedral(octets[b, ..., m], m)``."""
    o = octets(case)
    groups = []
    for modes in (ensemble.EVEN_MODES, ensemble.ODD_MODES):
        groups.append(_frozen(np.stack([np.ascontiguousarray(veval.dihedral(o[i, :, :, :, m], m).transpose(2, 0, 1))
                                        for i in range(o.shape[0]) for m in modes])))
    return tuple(groups)


def sums(case):
    """(sequential, pairwise) float32 sums of every octet, flat."""
    o = octets(case).reshape(-1, 8)
    seq = np.zeros(len(o), dtype=np.float32)
    for m in range(8):
        seq += o[:, m]
    pair = np.float32(0) + (((o[:, 0] + o[:, 1]) + (o[:, 2] + o[:, 3])) + ((o[:, 4] + o[:, 5]) + (o[:, 6] + o[:, 7])))
    return seq, pair


@functools.lru_cache(maxsize=None)
def expanded(case, dtype, flip=True):
    """``ensemble.expand_np`` of the case's uint8 ("u8") or float32 ("f32") source."""
    return tuple(None if a is None else _frozen(a) for a in ensemble.expand_np(source_u8(case) if dtype == "u8" else source_f32(case), flip))


@functools.lru_cache(maxsize=None)
def reduced(case, order, out, layout, flip=True):
    """``ensemble.reduce_np`` of the case's restored groups (without ``flip``: of the even group's first B images alone)."""
    even, odd = restored(case)
    return _frozen(ensemble.reduce_np(even, odd, order, out, layout) if flip else ensemble.reduce_np(even[:case[3]], None, order, out, layout))


def bits(a):
    """An array's raw bit pattern (float32 as int32: -0 and +0 differ, NaNs compare by payload)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(t, want):
    """A CUDA / CPU tensor equals a host array bit for bit, shape and dtype included."""
    got = t.detach().cpu().numpy()
    return got.shape == want.shape and got.dtype == want.dtype and bool((bits(got) == bits(want)).all())
