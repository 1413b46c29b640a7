#!/usr/bin/env python
"""Time of the device-side self-ensemble (virnet_amd/ensemble.py) on SIDD-shaped blocks (256 x 256 x 3 uint8), B = 1 and 4 blocks per call:

  kernels   ``expand`` and ``reduce`` alone, from device events (warm-up, then at least ``--seconds`` of timed calls): microseconds per
            call, and bytes moved / time next to the 6.29 TB/s a device copy reaches;
  paths     a whole block, uint8 on the host in -> uint8 on the host out, through the SIDD network (n_feat=[96,160,224,288], dep_S=8,
            sigma_chn=3, noise_avg=False, synthetic weights), two ways measured in ALTERNATING pairs (wall clock around a
            synchronisation): ``ensemble.restore`` with the orientations of the B blocks as one batch, and the path it replaces --
            ``eval.flip_ensemble`` around N = 1 forwards, then ``img_as_ubyte(clip(.))``, block after block.

Every (step, B) runs in a child process of its own under a time limit; the parent never opens the device and stops at the first step
that fails.  Prints one JSON line per step.

    python tools/bench_ensemble.py [--seconds 1.0] [--pairs 9]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29
H = W = 256
C = 3
CFG = dict(im_chn=3, sigma_chn=3, n_feat=[96, 160, 224, 288], dep_S=8, n_resblocks=3, noise_cond=True, extra_mode="Input", noise_avg=False)
STEP_LIMIT_S = {"kernels": 120, "paths": 240}


def _blocks(b):
    return np.random.default_rng(b).integers(0, 256, size=(b, H, W, C), dtype=np.uint8)


def _timed(step, seconds, warmup=5):
    import torch
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


def step_kernels(b, args):
    import torch
    from virnet_amd import ensemble
    src = torch.from_numpy(_blocks(b)).cuda()
    groups = ensemble.expand(src)
    small, large = b * H * W * C, 8 * b * C * H * W * 4              # the uint8 image; its eight float32 orientations
    row = {"step": "kernels", "blocks": b, "bytes_moved": small + large}
    for name, fn in (("expand", lambda: ensemble.expand(src)), ("reduce", lambda: ensemble.reduce(*groups))):
        ms = _timed(fn, args.seconds)
        row[name + "_us"] = round(ms * 1e3, 2)
        row[name + "_TBps"] = round((small + large) / (ms * 1e-3) / 1e12, 4)
        row[name + "_share_of_copy_rate"] = round(row[name + "_TBps"] / COPY_TBPS, 4)
    return row


def step_paths(b, args):
    import torch
    from virnet_amd import ensemble
    from virnet_amd import eval as veval
    from virnet_amd.networks import VIRAttResUNet
    from virnet_amd.utils.synth import synth_state_dict
    net = VIRAttResUNet(**CFG)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    blocks = _blocks(b)
    to_x = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)[None]))        # noqa: E731

    def new_path():
        with torch.no_grad():
            return ensemble.restore(lambda x: net(x)[0], blocks, batch=8 * b).cpu().numpy()

    def parent_path():
        out = []
        with torch.no_grad():
            for blk in blocks:
                mean = veval.flip_ensemble(lambda a: net(to_x(a).cuda())[0].squeeze(0).cpu().numpy().transpose(1, 2, 0), np.float32(blk / 255.0))
                out.append(veval.img_as_ubyte(np.clip(mean, 0, 1)))
        return np.stack(out)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / b, res

    for _ in range(3):                                               # warm-up: graph captures, allocator, kernel loading
        new_path(), parent_path()
    new_ms, old_ms, differing = [], [], 0
    for _ in range(args.pairs):
        t_new, got = wall(new_path)
        t_old, want = wall(parent_path)
        new_ms.append(t_new)
        old_ms.append(t_old)
        differing = int((got != want).sum())
    ratios = [o / n for o, n in zip(old_ms, new_ms)]
    return {"step": "paths", "blocks": b, "pairs": args.pairs, "new_ms_per_block_median": round(statistics.median(new_ms), 3),
            "parent_ms_per_block_median": round(statistics.median(old_ms), 3), "new_ms_per_block": [round(v, 3) for v in new_ms],
            "parent_ms_per_block": [round(v, 3) for v in old_ms], "parent_over_new_median": round(statistics.median(ratios), 3),
            "parent_over_new_min": round(min(ratios), 3), "pairs_where_new_is_not_slower": sum(r >= 1.0 for r in ratios),
            "bytes_differing_from_parent_path": differing, "bytes_per_result": int(blocks.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), help="(internal) run one step in this process")
    ap.add_argument("--blocks", type=int, default=1)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "bench_ensemble needs a ROCm device"
        print(json.dumps({"kernels": step_kernels, "paths": step_paths}[args.step](args.blocks, args)), flush=True)
        return 0
    for step in ("kernels", "paths"):
        for b in (1, 4):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--blocks", str(b), "--seconds", str(args.seconds),
                   "--pairs", str(args.pairs)]
            try:
                rc = subprocess.run(cmd, timeout=STEP_LIMIT_S[step]).returncode
            except subprocess.TimeoutExpired:
                print(f"bench_ensemble: step {step} B={b} ran into its {STEP_LIMIT_S[step]} s limit; stopping", file=sys.stderr)
                return 124
            if rc != 0:
                print(f"bench_ensemble: step {step} B={b} ended with status {rc}; stopping", file=sys.stderr)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
