"""Shared cases of the LPIPS tests (tests/test_lpips_host.py, test_lpips_gpu.py, test_redzone_lpips_gpu.py): synthetic weights at the true
AlexNet widths and the smallest shapes at which each stage can still go wrong.  The fp64 yardsticks are computed once and never modified."""
from functools import lru_cache

import numpy as np
import torch

from virnet_amd import lpips

SEED = 1234
# (H, W, N)
CASES = [(31, 31, 1),       # every map at its minimum (7 / 3 / 1), the deepest map 1 x 1
         (35, 47, 1),       # conv1's last window partly in the padding (35 = 4 * 7 + 7), non-square
         (63, 37, 2),       # deepest map 3 x 1
         (64, 64, 3),       # maps 15 / 7 / 3
         (97, 81, 1)]       # more than one tile in every kernel (23 x 19 = 437 pixels in conv1, 11 x 9 = 99 in conv2), odd everything
IDS = [f"{h}x{w}x{n}" for h, w, n in CASES]
EDGE_CASES = [CASES[0], CASES[1], CASES[4]]
EDGE_IDS = [IDS[0], IDS[1], IDS[4]]


@lru_cache(maxsize=None)
def weights():
    return lpips.synth_weights(SEED)


def pair_u8(case):
    """uint8 [N,3,H,W] a and b = a + noise: structure + texture, not white noise (tests/test_metrics_gpu.py:36-41)."""
    h, w, n = case
    rng = np.random.default_rng(h * 1000 + w * 10 + n)
    a = rng.integers(0, 256, size=(n, 3, h, w), dtype=np.uint8)
    a = (a // 4 + np.linspace(0, 190, w, dtype=np.float64)[None, None, None, :]).astype(np.uint8)
    b = np.clip(np.rint(a.astype(np.float64) + rng.standard_normal(a.shape) * 20.0), 0, 255).astype(np.uint8)
    return torch.from_numpy(a), torch.from_numpy(b)


def pair_f32(case):
    """float32 a in the networks' scale, outside [0,1] in places and with one NaN, and the uint8 b of :func:`pair_u8`."""
    h, w, n = case
    a, b = pair_u8(case)
    rng = np.random.default_rng(h * 1000 + w * 10 + n + 7)
    x = a.numpy().astype(np.float32) / np.float32(255.0) + (rng.standard_normal(a.shape) * 0.02).astype(np.float32)
    x[:, :, :2, :] -= np.float32(0.3)          # below 0 in the top rows
    x[:, :, -2:, :] += np.float32(0.3)         # above 1 in the bottom rows
    x[0, 1, h // 2, w // 3] = np.float32("nan")
    return torch.from_numpy(x), b


def pair(case, form):
    return pair_u8(case) if form == "u8" else pair_f32(case)


FORMS = ("u8", "f32")


@lru_cache(maxsize=None)
def reference(case, form):
    """(distance float64 [N], taps of a in float64) by the definition on the CPU."""
    a, b = pair(case, form)
    with torch.no_grad():
        return lpips.distance_torch(a, b, weights(), torch.float64), lpips.features_torch(a, weights(), torch.float64)


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and bool((x.cpu().view(torch.int64) == y.cpu().view(torch.int64)).all())
