#!/usr/bin/env python
"""Time of the real-noise training batch (virnet_amd/datagen.py: real_batch, mixup) at the reference configuration of
configs/denoising_real.json -- batch 16, patch 128, variance window 7 -- from a pool of seeded uint8 image pairs of 256 x 256 (the size of
the reference's pre-cut SIDD patches), in one process:

  * ``real``       (a) ``datagen.real_batch`` from host parameters and a host mix (their packing and uploads included): two launches;
  * ``today``      (b) the same result by what a user had to write before: ``datagen.pair_batch``, the mix in torch ops as
                   datasets/data_tools.py:19-30 writes it (two gathers, six elementwise launches), ``elbo.noise_estimate``;
  * ``mixup``      (c) ``datagen.mixup`` alone on two resident tensors of that shape, from a host mix;
  * ``mixup_torch``    the torch ops of (b)'s mix alone on the same tensors.

The parameters and the mix are drawn once, outside the timing, and shared.  Every figure is the median of ``--repeats`` timed blocks of
``--calls`` calls after warm-up, with the minimum and the maximum beside it; the routes alternate block by block.  Per route: wall time per
batch (host clock around a block that ends in a synchronise) and device time (events).  One JSON line per row; each row also states the one
bar of the comparison: the new route's median is not above the old route's median by more than the old route's own min-max spread.

``--kernels`` instead runs 3 + 10 calls of ``real`` and of ``mixup`` only, for ``rocprofv3 --kernel-trace --stats -- python
tools/bench_realbatch.py --kernels``; the row it prints holds the bytes each launch has to move.

    python tools/bench_realbatch.py [--repeats 9] [--calls 20]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

POOL_IMAGES, POOL_SHAPE = 64, (256, 256)
N, P, K = 16, 128, 7


def _pool_images(seed):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, POOL_SHAPE + (3,), dtype=np.uint8) for _ in range(POOL_IMAGES)]


def _block(step, calls):
    """(wall ms per call including the closing synchronise, device ms per call)"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        step()
    e1.record()
    e1.synchronize()
    wall = time.perf_counter() - t0
    return wall * 1e3 / calls, e0.elapsed_time(e1) / calls


def _ab(steps, repeats, calls, warmup=3):
    import torch
    for step in steps.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    ms = {name: [] for name in steps}
    for _ in range(repeats):
        for name, step in steps.items():
            ms[name].append(_block(step, calls))
    out = {}
    for name, v in ms.items():
        for kind, col in (("wall", [a for a, _ in v]), ("device", [b for _, b in v])):
            out[f"{kind}_ms_{name}"] = round(statistics.median(col), 4)
            out[f"{kind}_ms_{name}_range"] = [round(min(col), 4), round(max(col), 4)]
    return out


def _bar(row, new, old):
    """the one bar, on both clocks: median(new) <= median(old) + (max(old) - min(old))"""
    out = {}
    for kind in ("wall", "device"):
        lo, hi = row[f"{kind}_ms_{old}_range"]
        out[f"bar_{kind}_{new}_vs_{old}"] = bool(row[f"{kind}_ms_{new}"] <= row[f"{kind}_ms_{old}"] + (hi - lo))
    return out


def routes(dev):
    import torch
    from virnet_amd import datagen, elbo
    pool = datagen.ImagePool.paired(_pool_images(20241020), _pool_images(20241021), dev)
    params = datagen.draw_pair_params(random.Random(1), pool, N, P)
    torch.manual_seed(1)
    mix = datagen.draw_mixup_params(N)
    a, b = datagen.pair_batch(pool, params, P)          # (im_noisy, im_gt): the resident tensors of (c)

    def torch_mix(im_gt, im_noisy):
        # MixUp_AUG.aug with the draws taken from ``mix``
        indices = torch.from_numpy(mix.perm.astype(np.int64)).to(dev, non_blocking=True)
        lam = torch.from_numpy(mix.lam).to(dev, non_blocking=True).view(-1, 1, 1, 1)
        im_gt2, im_noisy2 = im_gt[indices], im_noisy[indices]
        return lam * im_gt + (1 - lam) * im_gt2, lam * im_noisy + (1 - lam) * im_noisy2

    def real():
        return datagen.real_batch(pool, params, P, mix, K)

    def today():
        im_noisy, im_gt = datagen.pair_batch(pool, params, P)
        im_gt, im_noisy = torch_mix(im_gt, im_noisy)
        return im_noisy, im_gt, elbo.noise_estimate(im_noisy, im_gt, K)

    def mixup():
        return datagen.mixup(b, a, mix)

    def mixup_torch():
        return torch_mix(b, a)

    same = all(torch.equal(x, y) for x, y in zip(real(), today())) and all(torch.equal(x, y) for x, y in zip(mixup(), mixup_torch()))
    plane = N * 3 * P * P
    moved = {"datagen_pair_mix_kernel": 4 * plane + 2 * 4 * plane, "noise_estimate_kernel": 3 * 4 * plane, "mixup_kernel": 6 * 4 * plane}
    info = dict(shape=[N, 3, P, P], k_size=K, pool=[POOL_IMAGES, *POOL_SHAPE, 3], routes_agree_bitwise=bool(same), bytes_per_launch=moved)
    return {"real": real, "today": today}, {"mixup": mixup, "mixup_torch": mixup_torch}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_realbatch needs a ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    batch, mix_only, info = routes(dev)
    if args.kernels:
        for step in (batch["real"], mix_only["mixup"]):
            for _ in range(13):
                step()
        torch.cuda.synchronize()
        print(json.dumps({"row": "kernels", "calls": 13, **info}), flush=True)
        return
    for row_name, steps, new, old in (("batch", batch, "real", "today"), ("mixup", mix_only, "mixup", "mixup_torch")):
        row = {"row": row_name, **info, "blocks": args.repeats, "calls_per_block": args.calls}
        row.update(_ab(steps, args.repeats, args.calls))
        row.update(_bar(row, new, old))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
