"""Shared cases of the MixUp tests (tests/test_mixup_host.py, tests/test_mixup_gpu.py, tests/test_redzone_mixup_gpu.py): one mix for the nine
samples of tests/datagen_cases.py and the numpy definitions' outputs for it, computed once per patch size.

The mix: sample 0 is a fixed point; samples 1 and 2 form a 2-cycle between augmentation flags 1 and 2, i.e. an untransposed tile paired with
a transposed one; samples 3..8 form a 6-cycle in which every sample's partner has another image, crop corner or flag, and 8 -> 3 share flag
3.  lam: one half, the two ends of the range (0: the partner alone, 1: the sample alone), the nearest values to them (nextafter(1, 0), where
1 - lam is one ulp; 2^-24), and four Beta(0.6, 0.6) draws."""
import functools

import numpy as np

import datagen_cases as dc
from virnet_amd import datagen

PERM = [0, 2, 1, 4, 5, 6, 7, 8, 3]
LAM = np.asarray([0.5, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), 2.0 ** -24, 0.7851624, 0.00165265, 0.4062881, 0.06652636],
                 dtype=np.float32)
# a second mix (a graph replay, reordered batches): another permutation (one 9-cycle), the weights rotated
PERM2 = [3, 0, 4, 1, 8, 2, 5, 6, 7]
LAM2 = np.roll(LAM, 4)
# shapes of the plain mix beside the golden (9,3,20,20): per odd (the 4-byte form), a tiny odd one, whole 16-byte rows
SHAPES = [(9, 3, 33, 33), (5, 1, 7, 3), (2, 3, 64, 64)]


@functools.lru_cache(maxsize=None)
def mix(second: bool = False) -> datagen.MixParams:
    return datagen.MixParams(PERM2 if second else PERM, LAM2 if second else LAM)


def mix_for(n: int, seed: int = 0) -> datagen.MixParams:
    """a mix for a batch of ``n``: a seeded permutation, lam from LAM (so the ends of the range stay in)"""
    g = np.random.default_rng(seed + n)
    return datagen.MixParams(g.permutation(n), g.permutation(LAM)[:n])


@functools.lru_cache(maxsize=None)
def tensors(shape, seed: int = 0):
    """two fp32 tensors of ``shape`` built as u8 * fp32(1/255).  Read-only."""
    g = np.random.default_rng(1000 + seed + int(np.prod(shape)))
    out = tuple(g.integers(0, 256, shape, dtype=np.uint8).astype(np.float32) * np.float32(1.0 / 255.0) for _ in range(2))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(p: int):
    """(im_noisy, im_gt) of real_batch_np for datagen_cases.params(p) and mix().  Read-only."""
    out = datagen.real_batch_np(list(dc.images(0)), list(dc.images(1)), dc.params(p), mix())
    for v in out:
        v.setflags(write=False)
    return out
