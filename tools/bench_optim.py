#!/usr/bin/env python
"""Time of the device optimizer (virnet_amd/optim.py) from device events, next to the torch routes it can replace, in one process:

  * ``isolated``: clip + Adam step on resident gradients for the parameters of bench.py's denoiser (configs/denoising_syn.json) and of its
    SISR x4 network: ``torch`` = one ``nn.utils.clip_grad_norm_`` per sub-network + default ``torch.optim.Adam.step()`` (what bench.py
    --optimizer times), ``fused`` = the same clips + ``Adam(fused=True)`` when this torch constructs it, ``clipadam`` =
    ``virnet_amd.optim.ClipAdam``.  Per route the device time per step and the host time to enqueue one step (no sync inside a block);
  * ``train_step``: the ``bench.py --task train --optimizer`` step (forward, objective, backward, clip + Adam; bench.py's network, data and
    prior) with each optimizer, and without one.

Every figure is the median of ``--repeats`` timed blocks of ``--calls`` calls after warm-up, with the minimum and the maximum of the blocks
beside it; the implementations alternate block by block.  Prints one JSON line per row.

``--launches ROUTE`` instead runs 10 isolated steps of one route on the denoiser after 3 warm-up steps and prints their count: under
``rocprofv3 --kernel-trace --stats -- python tools/bench_optim.py --launches ROUTE`` the kernel calls of the trace, less those of
``--launches none`` (set-up only), divided by 10 are the route's launches per step.

    python tools/bench_optim.py [--repeats 15] [--calls 20] [--dtype bf16]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLIPS = {"denoise": (("rnet", 1e3), ("snet", 1e2)),                       # train_denoising_syn.py:182-183
         "sisr": (("rnet", 5e2), ("snet", 1e2), ("knet", 5e2))}           # train_SISR.py:226-228 (as bench.py --task train_sisr)


def _block(step, calls):
    """(device ms per call, host ms per call to enqueue)"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(calls):
        step()
    host = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, host * 1e3 / calls


def _ab(steps, repeats, calls, warmup=5):
    """{name: {"device": (median, min, max), "host": (median, min, max)}} with the implementations alternating block by block"""
    import torch
    for step in steps.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    ms = {name: [] for name in steps}
    for _ in range(repeats):
        for name, step in steps.items():
            ms[name].append(_block(step, calls))
            torch.cuda.synchronize()
    out = {}
    for name, v in ms.items():
        dev, host = [a for a, _ in v], [b for _, b in v]
        out[name] = {"device": (statistics.median(dev), min(dev), max(dev)), "host": (statistics.median(host), min(host), max(host))}
    return out


def _put(row, res, kinds=("device", "host")):
    for impl, r in res.items():
        for kind in kinds:
            med, lo, hi = r[kind]
            row[f"{kind}_ms_{impl}"] = round(med, 4)
            row[f"{kind}_ms_{impl}_range"] = [round(lo, 4), round(hi, 4)]


def _groups(net, task):
    return [([p for n_, p in net.named_parameters() if key in n_.lower()], mx) for key, mx in CLIPS[task]]


def _routes(task, dev, which=("torch", "fused", "clipadam")):
    """{route: step()} on resident gradients, each over its own copy of the network's parameters"""
    import torch
    import bench
    from virnet_amd.optim import ClipAdam
    steps, info, notes = {}, {}, {}
    for route in which:
        net, sd = bench.build_net(dev, task)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev)
        params = list(net.parameters())
        groups = _groups(net, task)
        g = torch.Generator().manual_seed(3)
        for p in params:
            p.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(dev)
        info = {"tensors": len(params), "parameters": sum(p.numel() for p in params), "clip_sets": [len(m) for m, _ in groups]}
        if route == "clipadam":
            opt = ClipAdam(params, lr=2e-4, clip=groups)
            steps[route] = opt.step
            continue
        try:
            opt = torch.optim.Adam(params, lr=2e-4, **({"fused": True} if route == "fused" else {}))
        except Exception as e:                                  # (a torch build without the fused kernels: the row says so)
            notes["fused_unavailable"] = repr(e)
            continue

        def step(opt=opt, groups=groups):
            for members, mx in groups:
                torch.nn.utils.clip_grad_norm_(members, mx)
            opt.step()
        steps[route] = step
    return steps, {**info, **notes}


def isolated(task, repeats, calls):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    steps, info = _routes(task, dev)
    row = {"row": "isolated", "network": task, **info, "calls_per_block": calls, "blocks": repeats}
    _put(row, _ab(steps, repeats, calls))
    print(json.dumps(row), flush=True)


def train_step(repeats, calls, dtype, size=128, n=32):
    import torch
    import bench
    from virnet_amd.loss import elbo_denoising_simple
    from virnet_amd.optim import ClipAdam
    from virnet_amd.utils.synth import synth_images
    dev = torch.device("cuda", torch.cuda.current_device())
    x = synth_images(n, 3, size, size, seed=20240916).to(dev)
    gt = synth_images(n, 3, size, size, seed=7).to(dev)
    sigma_gt = (0.02 + 0.25 * synth_images(n, 1, size, size, seed=11).to(dev)) ** 2
    alpha0 = torch.tensor([0.5 * 7 ** 2], dtype=torch.float32, device=dev)
    beta0 = alpha0 * sigma_gt
    steps, losses = {}, {}
    for route in ("none", "torch", "clipadam"):
        net, sd = bench.build_net(dev, "denoise")
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).train()
        groups = _groups(net, "denoise")
        opt = {"none": None, "torch": torch.optim.Adam(net.parameters(), lr=2e-4) if route == "torch" else None,
               "clipadam": ClipAdam(net.parameters(), lr=2e-4, clip=groups) if route == "clipadam" else None}[route]

        def step(net=net, opt=opt, groups=groups, route=route):
            for p in net.parameters():
                p.grad = None
            mu, sig = net(x)
            loss = elbo_denoising_simple(mu, sig, x, gt, 1e-6, alpha0, beta0)[0]
            loss.backward()
            if route == "torch":
                for members, mx in groups:
                    torch.nn.utils.clip_grad_norm_(members, mx)
            if opt is not None:
                opt.step()
            return loss.detach()
        losses[route] = float(step())
        steps[route] = step
    row = {"row": "train_step", "shape": [n, 3, size, size], "dtype": dtype, "calls_per_block": calls, "blocks": repeats,
           **{f"first_loss_{k}": v for k, v in losses.items()}}
    _put(row, _ab(steps, repeats, calls, warmup=3), kinds=("device",))
    print(json.dumps(row), flush=True)


def launches(route):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    steps, _ = _routes("denoise", dev, which=() if route == "none" else (route,))
    n = 0
    for name, step in steps.items():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        for _ in range(10):
            step()
            n += 1
    torch.cuda.synchronize()
    print(json.dumps({"row": "launches", "route": route, "warmup_steps": 3 if n else 0, "steps": n}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--step-calls", type=int, default=5, help="training steps per timed block")
    ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"], help="conv operand form of the training step, as bench.py --dtype")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--launches", default=None, choices=["none", "torch", "fused", "clipadam"])
    args = ap.parse_args()
    if args.dtype == "bf16":
        os.environ["VIRNET_CONV_FORM"] = "bf16"          # (process state, read when the convs are first planned: set before any import)
    import torch
    assert torch.cuda.is_available(), "bench_optim needs a ROCm device"
    if args.launches:
        launches(args.launches)
        return
    for task in ("denoise", "sisr"):
        isolated(task, args.repeats, args.calls)
    if not args.skip_train:
        train_step(args.repeats, args.step_calls, args.dtype)


if __name__ == "__main__":
    main()
