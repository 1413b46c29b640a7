#!/usr/bin/env python
"""Time of the weight average's two launches (virnet_amd/ema.py, csrc/ema.hip) on the parameter lists of the three shipped networks --
denoise-syn, denoise-real and SISR (tools/testing_demo.py's configurations) -- next to what they replace and to the byte floor:

  * ``update``: ``WeightEMA.update()`` -- reads the shadow and the parameter, writes the shadow: three streams of 4 bytes per element;
  * ``swap``: ``WeightEMA.swap()`` -- reads and writes both: four streams;
  * ``foreach_lerp``: ``torch._foreach_lerp_(shadows, parameters, w)`` on the same tensors;
  * ``copy3`` / ``copy4``: one ``copy_`` between two flat buffers sized so that it moves the update's three (the swap's four) streams of
    bytes: the floor at the device's copy rate.

Each route is warmed up, then timed with HIP events around ``--reps`` back-to-back calls (at least 200), ``--blocks`` times; the figure
is the median block's time per call.  Such a block is bound by the slower of the device and the host that enqueues it, so the host's own
time per call (the clock around the same calls, no synchronisation inside) is printed beside it.  One JSON line per parameter list.

    python tools/bench_ema.py [--reps 200] [--blocks 5] [--decay 0.999]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(torch, call, reps, blocks):
    """(median device µs per call over the blocks, median host µs per call)"""
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    dev_us, host_us = [], []
    for _ in range(blocks):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        for _ in range(reps):
            call()
        end.record()
        host_us.append(1e6 * (time.perf_counter() - t0) / reps)
        end.synchronize()
        dev_us.append(1e3 * start.elapsed_time(end) / reps)
    return statistics.median(dev_us), statistics.median(host_us)


def measure(task, reps, blocks, decay):
    import torch
    from testing_demo import TASKS
    from virnet_amd.ema import WeightEMA, weight_at
    cls, kw = TASKS[task]
    shapes = [(name, tuple(p.shape)) for name, p in cls(**kw).named_parameters()]
    g = torch.Generator().manual_seed(1)
    params = [(name, torch.nn.Parameter((0.1 * torch.randn(shape, generator=g)).cuda())) for name, shape in shapes]
    avg = WeightEMA(params, decay=decay)
    with torch.no_grad():
        for s in avg.shadows:
            s.mul_(0.5)
    n = sum(p.numel() for p in avg.params)
    w = weight_at(0, decay)
    flat = {k: (torch.empty(k * n // 2, device="cuda"), torch.randn(k * n // 2, device="cuda")) for k in (3, 4)}
    routes = {
        "update": avg.update,
        "swap": avg.swap,
        "foreach_lerp": lambda: torch._foreach_lerp_(avg.shadows, [p.detach() for p in avg.params], w),
        "copy3": lambda: flat[3][0].copy_(flat[3][1]),
        "copy4": lambda: flat[4][0].copy_(flat[4][1]),
    }
    row = {"row": "ema", "task": task, "tensors": len(avg.params), "elements": n, "mbytes_per_stream": round(4e-6 * n, 1), "decay": decay,
           "reps": reps, "blocks": blocks}
    with torch.no_grad():
        for name, call in routes.items():
            dev_us, host_us = _timed(torch, call, reps, blocks)
            row[f"{name}_us"], row[f"{name}_host_us"] = round(dev_us, 1), round(host_us, 1)
    assert not avg.swapped                                     # (an even number of swaps)
    row["update_over_copy3"] = round(row["update_us"] / row["copy3_us"], 2)
    row["update_over_foreach_lerp"] = round(row["update_us"] / row["foreach_lerp_us"], 2)
    row["swap_over_copy4"] = round(row["swap_us"] / row["copy4_us"], 2)
    row["update_gbytes_per_s"] = round(3 * 4 * n / row["update_us"] * 1e-3, 1)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="calls per timed block (even, at least 200)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--tasks", nargs="+", default=["denoising-syn", "denoising-real", "sisr"])
    args = ap.parse_args()
    if args.reps < 200 or args.reps % 2:
        ap.error("--reps: an even number of at least 200 calls")
    import torch
    assert torch.cuda.is_available(), "bench_ema needs a ROCm device"
    for task in args.tasks:
        measure(task, args.reps, args.blocks, args.decay)


if __name__ == "__main__":
    main()
