#!/usr/bin/env python
"""Time of the device metrics (virnet_amd/metrics.py) per call, from device events (warm-up, at least ``--seconds`` of timed calls per
config), next to two yardsticks: the host functions of virnet_amd/eval.py on the same data on this machine, and the time to read both
inputs once at the 6.29 TB/s a device copy reaches (entry-conv row).  Prints one JSON line per config.

    python tools/bench_metrics.py                 481x321 RGB pair and 32 x 256^2 x 3, RGB and Y, uint8 and float32 restored image
    python tools/bench_metrics.py --no-host       device times only (for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virnet_amd import eval as veval, metrics  # noqa: E402

COPY_TBPS = 6.29


def _timed(step, seconds, warmup=5):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, ms = 0, 0.0
    while ms < seconds * 1e3:
        e0.record()
        for _ in range(50):
            step()
        e1.record()
        e1.synchronize()
        ms += e0.elapsed_time(e1)
        calls += 50
    return ms / calls


def fp64_fma(n, cm, hc, wc):
    """fp64 multiply-adds the tiled separable filter executes: per 32 x 32 tile 42 rows x 32 columns (horizontal) + 32 x 32 (vertical),
    5 quantities x 11 taps each."""
    tiles = -(-(hc - 10) // 32) * -(-(wc - 10) // 32)
    return n * cm * tiles * (42 * 32 + 32 * 32) * 5 * 11


def config(n, h, w, border, ycbcr, float_mu, seconds, host):
    g = torch.Generator().manual_seed(1)
    gt = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8)
    mu = (gt.float() / 255.0 + torch.randn(n, 3, h, w, generator=g) * (10 / 255.0))
    a = (mu if float_mu else torch.from_numpy(veval.img_as_ubyte(mu.numpy()))).cuda()
    b = gt.cuda()
    ms = _timed(lambda: metrics.psnr_ssim(a, b, border=border, ycbcr=ycbcr), seconds)
    ms_psnr = _timed(lambda: metrics.psnr_ssim(a, b, border=border, ycbcr=ycbcr, with_ssim=False), seconds)
    nbytes = a.numel() * a.element_size() + b.numel()
    row = {"n": n, "h": h, "w": w, "border": border, "ycbcr": ycbcr, "restored_dtype": "float32" if float_mu else "uint8",
           "device_ms_per_call": round(ms, 5), "device_ms_psnr_only": round(ms_psnr, 5), "input_bytes": nbytes,
           "read_once_ms_at_6.29TBps": round(nbytes / (COPY_TBPS * 1e12) * 1e3, 6),
           "fp64_fma": fp64_fma(n, 1 if ycbcr else 3, h - 2 * border, w - 2 * border)}
    row["fp64_gfma_per_s"] = round(row["fp64_fma"] / (ms * 1e-3) / 1e9, 1)
    if host:
        mu_hwc = mu.numpy().transpose(0, 2, 3, 1)
        gt_hwc = np.ascontiguousarray(gt.numpy().transpose(0, 2, 3, 1))
        t = {"img_as_ubyte": 0.0, "psnr": 0.0, "ssim": 0.0}
        for i in range(n):
            t0 = time.perf_counter()
            den = veval.img_as_ubyte(np.clip(mu_hwc[i], 0.0, 1.0))
            t1 = time.perf_counter()
            (veval.calculate_psnr_y if ycbcr else veval.calculate_psnr)(den, gt_hwc[i], border)
            t2 = time.perf_counter()
            veval.calculate_ssim(den, gt_hwc[i], border, ycbcr=ycbcr)
            t3 = time.perf_counter()
            t["img_as_ubyte"] += t1 - t0
            t["psnr"] += t2 - t1
            t["ssim"] += t3 - t2
        row["host_ms"] = {k: round(v * 1e3, 3) for k, v in t.items()}
        row["host_ms_total"] = round(sum(t.values()) * 1e3, 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics needs a ROCm device"
    for (n, h, w) in [(1, 481, 321), (32, 256, 256)]:
        for border, ycbcr in [(0, False), (16, True)]:
            for float_mu in (False, True):
                config(n, h, w, border, ycbcr, float_mu, args.seconds, not args.no_host and not float_mu)


if __name__ == "__main__":
    main()
