#!/usr/bin/env python
"""Time of one training batch's synthesis (virnet_amd/datagen.py) by three routes, in one process, at the shapes of bench.py's ``train``
(32 x 3 x 128^2 denoiser patches) and ``train_sisr`` (16 HR patches of 256^2, x4, k 21) configurations:

  * ``device``: ``datagen.denoise_batch`` / ``datagen.sisr_batch`` from host parameters (their packing and upload included), noise drawn on the
    device;
  * ``torch``:  the same batch by torch ops on the device -- index, ``flip`` / ``rot90``, ``torch.randn``, the sigma map and the blur kernels
    by broadcasting in fp64 -- ending, for SISR, in the same ``degrade.synthesize_lr``;
  * ``host``:   the numpy definitions (``denoise_batch_np`` / ``sisr_batch_np``, i.e. the reference's per-sample work in one process, with
    ``torch.randn`` on the CPU) followed by the uploads of the batch.

The parameters are drawn once, outside the timing, and shared.  Every figure is the median of ``--repeats`` timed blocks of ``--calls``
calls (``--host-calls`` for the host route) after warm-up, with the minimum and the maximum beside it; the routes alternate block by block.
Per route: wall time per batch (host clock around a block that ends in a synchronise) and device time (events).  One JSON line per row.

``--kernels TASK`` instead runs 3 + 10 calls of the device route only, for ``rocprofv3 --kernel-trace --stats -- python
tools/bench_datagen.py --kernels denoise``; the row it prints holds the bytes each launch has to move.

    python tools/bench_datagen.py [--repeats 9] [--calls 20] [--host-calls 1]
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

POOL_IMAGES, POOL_SHAPE = 64, (321, 481)          # BSD-sized images: 64 x 463 KB
DENOISE = dict(n=32, p=128)
SISR = dict(n=16, p=256, sf=4, k=21)


def _pool_images():
    g = np.random.default_rng(20240916)
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
    for name, step in steps.items():
        for _ in range(1 if name == "host" else warmup):
            step()
    torch.cuda.synchronize()
    ms = {name: [] for name in steps}
    for _ in range(repeats):
        for name, step in steps.items():
            ms[name].append(_block(step, calls[name]))
    out = {}
    for name, v in ms.items():
        for kind, col in (("wall", [a for a, _ in v]), ("device", [b for _, b in v])):
            out[f"{kind}_ms_{name}"] = round(statistics.median(col), 4)
            out[f"{kind}_ms_{name}_range"] = [round(min(col), 4), round(max(col), 4)]
    return out


def _augment_t(x, flag):
    """util_image.data_aug_np on a [C,H,W] tensor"""
    import torch
    x = torch.rot90(x, flag >> 1, (1, 2))
    return torch.flip(x, (1,)) if flag & 1 else x


def denoise_routes(images, dev):
    import torch
    from virnet_amd import datagen
    n, p = DENOISE["n"], DENOISE["p"]
    pool = datagen.ImagePool(images, dev)
    params = datagen.draw_denoise_params(random.Random(1), pool, n, p)
    dev_images = [torch.from_numpy(im).to(dev) for im in images]
    state = {"id": 0}

    def device():
        state["id"] += n
        return datagen.denoise_batch(pool, params, p, 7, base_id=state["id"])

    def torch_ops():
        f64 = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev, non_blocking=True).view(n, 1, 1)
        ch, cw, scale, up, down = (f64(v) for v in (params.center_h, params.center_w, params.scale, params.up, params.down))
        ii = torch.arange(p, dtype=torch.float64, device=dev).view(1, p, 1)
        jj = torch.arange(p, dtype=torch.float64, device=dev).view(1, 1, p)
        kk = torch.exp((-(ii - ch) ** 2 - (jj - cw) ** 2) / (2 * scale ** 2))
        lo, hi = kk.amin((1, 2), keepdim=True), kk.amax((1, 2), keepdim=True)
        sigma = (down + (kk - lo) / (hi - lo) * (up - down)).float().unsqueeze(1)
        gt = torch.stack([dev_images[params.img[i]][params.ind_h[i]:params.ind_h[i] + p, params.ind_w[i]:params.ind_w[i] + p].permute(2, 0, 1)
                          for i in range(n)]).float() * (1.0 / 255.0)
        noisy = gt + torch.randn(n, 3, p, p, device=dev) * sigma
        flags = params.flag.tolist()
        noisy, gt, sigma = (torch.stack([_augment_t(t[i], flags[i]) for i in range(n)]) for t in (noisy, gt, sigma))
        return noisy, gt, torch.clamp_min(sigma * sigma, 1e-10)

    def host():
        noise = torch.randn(n, 3, p, p).numpy()
        return tuple(torch.from_numpy(a).to(dev) for a in datagen.denoise_batch_np(images, params, noise))

    moved = n * p * p * (3 + 7 * 4)          # the crops' bytes read, seven fp32 planes written
    return {"device": device, "torch": torch_ops, "host": host}, dict(shape=[n, 3, p, p], bytes_per_launch={"datagen_patch_kernel<0>": moved})


def sisr_routes(images, dev):
    import torch
    from virnet_amd import datagen, degrade
    n, p, sf, k = SISR["n"], SISR["p"], SISR["sf"], SISR["k"]
    pool = datagen.ImagePool(images, dev)
    params = datagen.draw_sisr_params(random.Random(2), pool, n, p, sf)
    dev_images = [torch.from_numpy(im).to(dev) for im in images]
    degrade.warm_taps(p, p, sf, dev)
    state = {"id": 0}

    def device():
        state["id"] += n
        return datagen.sisr_batch(pool, params, p, sf, k, 7, base_id=state["id"])

    def torch_ops():
        f64 = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev, non_blocking=True)
        l1, l2, th = f64(params.lam1 ** 2), f64(params.lam2 ** 2), f64(params.theta)
        c, s = torch.cos(th), torch.sin(th)
        s00, s01, s11 = c * c * l1 + s * s * l2, c * s * (l1 - l2), s * s * l1 + c * c * l2
        det = s00 * s11 - s01 * s01
        g = torch.arange(k, dtype=torch.float64, device=dev) - k // 2
        dx, dy = g.view(1, 1, k), g.view(1, k, 1)
        q = -0.5 * ((s11 / det).view(n, 1, 1) * dx * dx - 2 * (s01 / det).view(n, 1, 1) * dx * dy + (s00 / det).view(n, 1, 1) * dy * dy)
        kernel = torch.softmax(q.view(n, -1), 1).view(n, 1, k, k).float()
        kinfo = torch.stack([s00, s11, s01 / (s00.sqrt() * s11.sqrt())], 1).float()
        flags = params.flag.tolist()
        hr = torch.stack([_augment_t(dev_images[params.img[i]][params.ind_h[i]:params.ind_h[i] + p, params.ind_w[i]:params.ind_w[i] + p].permute(2, 0, 1),
                                     flags[i]) for i in range(n)]).float() / 255.0
        std = torch.from_numpy(params.std.astype(np.float32)).to(dev, non_blocking=True)
        lr, blur = degrade.synthesize_lr(hr, kernel, sf, torch.randn(n, 3, p // sf, p // sf, device=dev), std)
        return hr, lr, blur, kinfo, std.view(n, 1, 1, 1)

    def host():
        noise = torch.randn(n, 3, p // sf, p // sf).numpy()
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in datagen.sisr_batch_np(images, params, sf, k, noise))

    moved = {"datagen_patch_kernel<2>": n * p * p * (3 + 3 * 4), "datagen_blur_kernel": n * (24 + 4 * (k * k + 3)),
             "datagen_normal_kernel": n * 3 * (p // sf) ** 2 * 4}
    return {"device": device, "torch": torch_ops, "host": host}, dict(shape=[n, 3, p, p], sf=sf, k_size=k, bytes_per_launch=moved)


TASKS = {"denoise": denoise_routes, "sisr": sisr_routes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--tasks", default="denoise,sisr")
    ap.add_argument("--kernels", default=None, choices=sorted(TASKS))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_datagen needs a ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    images = _pool_images()
    if args.kernels:
        steps, info = TASKS[args.kernels](images, dev)
        for _ in range(13):
            steps["device"]()
        torch.cuda.synchronize()
        print(json.dumps({"row": "kernels", "task": args.kernels, "calls": 13, **info}), flush=True)
        return
    for task in args.tasks.split(","):
        steps, info = TASKS[task](images, dev)
        calls = {"device": args.calls, "torch": args.calls, "host": args.host_calls}
        row = {"row": "batch", "task": task, **info, "pool": [POOL_IMAGES, *POOL_SHAPE, 3], "blocks": args.repeats, "calls_per_block": calls}
        row.update(_ab(steps, args.repeats, calls))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
