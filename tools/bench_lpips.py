#!/usr/bin/env python
"""Time of the device-side LPIPS (virnet_amd/lpips.py ``distance``) at the SISR table's sizes -- 480 x 320 and 320 x 480 pairs, N = 1 -- and
at 256 x 256 with N = 1 and 8, synthetic weights, float32 SR image against a uint8 ground truth as the table calls it.

The comparison is the same definition in torch ops on the device (``distance_torch`` in float32: torch's own convolutions and pools), in
the same process: ``--rounds`` ALTERNATING rounds, each a device-event time over ``--calls`` back-to-back calls of one path and then of the
other, after a warm-up.  If torch's convolutions do not run on the device the row says so and carries the kernels' time alone.  Every
row also has the time of the call replayed from a captured graph, the nine kernels back to back with no host work between them: equal to
the eager time when the device, not the host's enqueueing, bounds the call.

Every size runs in a child process of its own under a time limit; the parent never opens the device and stops at the first size that
fails.  Prints one JSON line per size and writes the lines to profiles/lpips_device_bench.jsonl (``--out``).

    python tools/bench_lpips.py [--rounds 9] [--calls 20]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((480, 320, 1), (320, 480, 1), (256, 256, 1), (256, 256, 8))          # (H, W, N)
STEP_LIMIT_S = 180
FLOP_PER_MAC = 2


def flops_per_pair(h, w):
    from virnet_amd import lpips
    return 2 * sum(FLOP_PER_MAC * hh * ww * co * ci * k * k for (hh, ww), (co, ci, k, _, _) in zip(lpips.map_sizes(h, w), lpips.CONVS))


def _images(h, w, n):
    rng = np.random.default_rng(h * 7 + w * 3 + n)
    gt = rng.integers(0, 256, size=(n, 3, h, w), dtype=np.uint8)
    gt = (gt // 4 + np.linspace(0, 190, w, dtype=np.float64)[None, None, None, :]).astype(np.uint8)
    sr = (gt.astype(np.float32) / np.float32(255.0) + (rng.standard_normal(gt.shape) * 0.05).astype(np.float32))      # un-clipped, like mu
    return sr, gt


def _event_ms(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def run_size(h, w, n, args):
    import torch
    from virnet_amd import _native, lpips
    weights = lpips.synth_weights(1234)
    sr, gt = _images(h, w, n)
    a, b = torch.from_numpy(sr).cuda(), torch.from_numpy(gt).cuda()
    row = {"h": h, "w": w, "n": n, "rounds": args.rounds, "calls_per_round": args.calls, "gflop_per_call": round(n * flops_per_pair(h, w) / 1e9, 3)}

    def ours():
        return lpips.distance(a, b, weights)

    def theirs():
        return lpips.distance_torch(a, b, weights, torch.float32)

    d = ours()
    baseline = True
    try:
        t = theirs()
        torch.cuda.synchronize()
        row["device_vs_torch_rel"] = float(((d.cpu() - t.double().cpu()).abs() / t.double().cpu()).max())
    except RuntimeError as e:                                        # torch's convolutions are not available on this device
        baseline = False
        row["torch_baseline"] = f"not run: {str(e).splitlines()[0][:160]}"
    for _ in range(args.warmup):
        ours()
        if baseline:
            theirs()
    torch.cuda.synchronize()
    ours_ms, torch_ms = [], []
    for _ in range(args.rounds):
        ours_ms.append(_event_ms(ours, args.calls))
        if baseline:
            torch_ms.append(_event_ms(theirs, args.calls))
    row["device_ms_median"] = round(statistics.median(ours_ms), 4)
    row["device_ms_min_max"] = [round(min(ours_ms), 4), round(max(ours_ms), 4)]
    row["device_tflops"] = round(row["gflop_per_call"] / statistics.median(ours_ms), 3)
    if baseline:
        ratios = [t / o for t, o in zip(torch_ms, ours_ms)]
        row["torch_ms_median"] = round(statistics.median(torch_ms), 4)
        row["torch_ms_min_max"] = [round(min(torch_ms), 4), round(max(torch_ms), 4)]
        row["torch_over_device_median"] = round(statistics.median(ratios), 3)
        row["torch_over_device_min_max"] = [round(min(ratios), 3), round(max(ratios), 3)]
        row["rounds_where_device_is_not_slower"] = sum(r >= 1.0 for r in ratios)
    # the kernels alone: the same call replayed from a captured graph, where no host work lies between the launches
    graph = torch.cuda.CUDAGraph()
    with _native.capture_lock, torch.cuda.graph(graph):
        ours()
    graph.replay()
    torch.cuda.synchronize()
    replay_ms = [_event_ms(graph.replay, args.calls) for _ in range(args.rounds)]
    row["device_graph_replay_ms_median"] = round(statistics.median(replay_ms), 4)
    row["device_graph_replay_ms_min_max"] = [round(min(replay_ms), 4), round(max(replay_ms), 4)]
    row["device_graph_replay_tflops"] = round(row["gflop_per_call"] / statistics.median(replay_ms), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_device_bench.jsonl"))
    ap.add_argument("--size", type=int, nargs=3, metavar=("H", "W", "N"), help="(internal) run one size in this process")
    args = ap.parse_args()
    if args.size:
        import torch
        assert torch.cuda.is_available(), "bench_lpips needs a ROCm device"
        print(json.dumps(run_size(*args.size, args)), flush=True)
        return 0
    lines = []
    for h, w, n in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(h), str(w), str(n), "--rounds", str(args.rounds), "--calls", str(args.calls),
               "--warmup", str(args.warmup)]
        try:
            res = subprocess.run(cmd, timeout=STEP_LIMIT_S, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"bench_lpips: {h}x{w} N={n} ran into its {STEP_LIMIT_S} s limit; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:
            print(f"bench_lpips: {h}x{w} N={n} ended with status {res.returncode}; stopping", file=sys.stderr)
            return res.returncode if res.returncode > 0 else 1
        lines += [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
