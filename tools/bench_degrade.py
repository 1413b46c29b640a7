#!/usr/bin/env python
"""Time of the device degradation (virnet_amd/degrade.py) from device events, next to the routes it can replace, in one process:

  * the training operator at the ``bench.py --task train_sisr`` shape (16 x 3 x 256 x 256, k = 21, sf = 4, "Bicubic" and "Direct"):
    ``loss.blur_downsample(impl="hip")`` against ``impl="torch"`` (reflect pad + torch.fft + dense tap matrices, the default), forward
    alone and forward + both gradients;
  * the evaluation input per Set5 image (x4, kernel 6 of the seven): ``degrade.degrade_lr`` (upload, launches, seeded host noise, the
    result left on the device; host clock around a device synchronise) against ``sisr_eval.degrade`` (scipy + numpy, host clock).

Every figure is the median of ``--repeats`` timed blocks after warm-up; the two implementations alternate block by block.  Prints one JSON
line per row.

    python tools/bench_degrade.py [--repeats 15] [--calls 20] [--data tests/golden/set5]
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virnet_amd import degrade, loss, sisr_eval  # noqa: E402
from virnet_amd import eval as veval  # noqa: E402


def _block_ms(step, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def _ab(steps, repeats, calls, warmup=5):
    """{name: (median ms per call, min, max)} with the implementations alternating block by block"""
    for step in steps.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    ms = {name: [] for name in steps}
    for _ in range(repeats):
        for name, step in steps.items():
            ms[name].append(_block_ms(step, calls))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def training_operator(repeats, calls):
    n, c, hw, k, sf = 16, 3, 256, 21, 4
    g = torch.Generator().manual_seed(1)
    x = torch.rand(n, c, hw, hw, generator=g).cuda().requires_grad_(True)
    ker = torch.rand(n, 1, k, k, generator=g)
    ker = (ker / ker.sum((2, 3), keepdim=True)).cuda().requires_grad_(True)
    gy = torch.randn(n, c, hw // sf, hw // sf, generator=g).cuda()
    for down in ("Bicubic", "Direct"):
        def forward(impl):
            with torch.no_grad():
                return loss.blur_downsample(x, ker, sf, down, impl=impl)

        def both(impl):
            return torch.autograd.grad(loss.blur_downsample(x, ker, sf, down, impl=impl), [x, ker], gy)

        diff = float((forward("hip") - forward("torch")).abs().max())
        gh, gt = both("hip"), both("torch")
        row = {"row": "training_operator", "shape": [n, c, hw, hw], "k": k, "sf": sf, "downsampler": down, "calls_per_block": calls,
               "blocks": repeats, "forward_max_abs_diff": diff, "gx_max_abs_diff": float((gh[0] - gt[0]).abs().max()),
               "gk_max_rel_diff": float((gh[1] - gt[1]).abs().max() / gt[1].abs().max())}
        for what, fn in (("forward", forward), ("forward_and_gradients", both)):
            res = _ab({"hip": lambda: fn("hip"), "torch": lambda: fn("torch")}, repeats, calls)
            for impl, (med, lo, hi) in res.items():
                row[f"{what}_ms_{impl}"] = round(med, 4)
                row[f"{what}_ms_{impl}_range"] = [round(lo, 4), round(hi, 4)]
        print(json.dumps(row), flush=True)


def eval_degradation(folder, repeats):
    sf = 4
    kernel = sisr_eval.test_kernels(sf)[5]
    for f in sorted(glob.glob(os.path.join(folder, "*.bmp"))):
        gt = sisr_eval.modcrop(veval.imread_rgb_uint8(f), sf)
        im = veval.img_as_float32(gt)
        row = {"row": "eval_degradation", "image": os.path.basename(f), "shape": list(im.shape), "sf": sf, "blocks": repeats}
        for down in ("bicubic", "direct"):
            dev = degrade.degrade_lr(im, kernel, sf, downsampler=down)            # warm-up: tap tables, code objects
            host = sisr_eval.degrade(im, kernel, sf, downsampler=down)
            row[f"{down}_max_abs_diff"] = float((dev[0].permute(1, 2, 0).cpu() - torch.from_numpy(host)).abs().max())
            t_dev, t_host = [], []
            for i in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                degrade.degrade_lr(im, kernel, sf, downsampler=down)
                torch.cuda.synchronize()
                t_dev.append((time.perf_counter() - t0) * 1e3)
                if i < max(3, repeats // 5):                                     # the host route takes ~1 s per image: fewer repeats
                    t0 = time.perf_counter()
                    sisr_eval.degrade(im, kernel, sf, downsampler=down)
                    t_host.append((time.perf_counter() - t0) * 1e3)
            row[f"{down}_ms_device"] = round(statistics.median(t_dev), 3)
            row[f"{down}_ms_host"] = round(statistics.median(t_host), 3)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--data", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "set5"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_degrade needs a ROCm device"
    training_operator(args.repeats, args.calls)
    eval_degradation(args.data, args.repeats)


if __name__ == "__main__":
    main()
