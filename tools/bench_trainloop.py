#!/usr/bin/env python
"""Images per second of the denoising training loop on the device (virnet_amd/fit.py), next to the loop a user writes from the README, in
one process, on bench.py's denoiser (configs/denoising_syn.json) at 128 x 128, batch 16 (the shipped configuration) and batch 32:

  * ``readme``: the README's loop body -- ``datagen.denoise_batch``, forward, ``elbo.elbo_denoising``, backward, ``ClipAdam.step()`` --
    with the reference's per-step host reads (train_denoising_syn.py:187-198: four ``.item()`` calls and the two gradient norms);
  * ``fit``: ``fit.train_step`` -- the same launches plus the ``StepLog`` push -- with the log read once per ``--read-every`` steps;
  * ``bench_train``: the region ``bench.py --task train`` times (forward, objective, backward on a fixed batch; no batch synthesis, no
    optimizer), for scale;
  * ``fit_ema`` (only with ``--ema-decay X``): ``fit`` plus ``ema.WeightEMA.update()`` after every step -- what ``fit_denoising`` adds per
    step with ``ema_decay``; ``ema_added_ms_per_step`` is its median step time less ``fit``'s, from the same alternating blocks.

A block is ``--calls`` steps between two device synchronisations, timed on the host clock (the host reads are the subject, so device events
alone would not do); the routes alternate block by block, ``--repeats`` blocks each after warm-up.  Per route the median images/s with the
minimum and the maximum of the blocks; ``spread_readme`` is (max - min) / median of the ``readme`` blocks, the yardstick for "not slower":
``fit`` passes when its median is not below the ``readme`` median by more than that spread.  Prints one JSON line per batch size.

``--launches ROUTE`` instead runs 10 steps of one route at batch 16 after 3 warm-up steps (``none``: the set-up only): under
``rocprofv3 --kernel-trace --stats -- python tools/bench_trainloop.py --launches ROUTE`` the kernel calls of the trace, less those of
``--launches none``, divided by the 13 traced steps (the warm-up steps, with the first step's one-off packing, are in the trace) are the
route's launches per step, by kernel name.

    python tools/bench_trainloop.py [--repeats 7] [--calls 100] [--dtype bf16]
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

CFG = dict(patch_size=128, epochs=120, warmup_epochs=5, lr=1e-4, lr_min=1e-6, print_freq=100, clip_grad_R=1e3, clip_grad_S=1e2, var_window=7,
           eps2=1e-6, steps_per_epoch=10000)          # configs/denoising_syn.json


def _pool(dev, count=16, size=256):
    import numpy as np
    from virnet_amd import datagen
    g = np.random.default_rng(20240916)
    return datagen.ImagePool([g.integers(0, 256, (size, size, 3), dtype=np.uint8) for _ in range(count)], dev)


def _routes(dev, batch, read_every, which=("readme", "fit", "bench_train"), ema_decay=None):
    """{route: run(calls)} each over its own copy of the network; run() enqueues `calls` steps with the route's own host reads"""
    import torch
    import bench
    from virnet_amd import datagen, elbo, fit
    from virnet_amd.loss import elbo_denoising_simple
    from virnet_amd.ema import WeightEMA
    from virnet_amd.optim import ClipAdam
    from virnet_amd.trainlog import StepLog
    from virnet_amd.utils.synth import synth_images
    c = fit.read_config(dict(CFG, batch_size=batch))
    pool = _pool(dev)
    alpha0 = (0.5 * torch.tensor([c["var_window"] ** 2], dtype=torch.float32)).to(dev)
    runs = {}
    for route in which:
        net, sd = bench.build_net(dev, "denoise")
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).train()
        p_r, p_s = fit.clip_sets(net)
        opt = ClipAdam(net.parameters(), lr=c["lr"], clip=[(p_r, c["clip_grad_R"]), (p_s, c["clip_grad_S"])])
        rng = random.Random(0)
        state = {"ii": 0, "acc": [0.0] * 4}
        if route == "readme":
            def run(calls, net=net, opt=opt, rng=rng, state=state):
                for _ in range(calls):
                    ii = state["ii"]
                    params = datagen.draw_denoise_params(rng, pool, batch, c["patch_size"])
                    im_noisy, im_gt, sigma_gt = datagen.denoise_batch(pool, params, c["patch_size"], seed=0, base_id=ii * batch)
                    beta0 = alpha0 * sigma_gt
                    opt.zero_grad()
                    mu, sigma = net(im_noisy)
                    loss, lh, kl_g, kl_ig = elbo.elbo_denoising(mu, sigma, im_noisy, im_gt, c["eps2"], alpha0, beta0)
                    loss.backward()
                    opt.step()
                    for k, v in enumerate((loss, lh, kl_g, kl_ig)):          # train_denoising_syn.py:187-190
                        state["acc"][k] += v.item() / c["steps_per_epoch"]
                    state["norms"] = (float(opt.grad_norms[0]), float(opt.grad_norms[1]))          # :197-198 (clip_grad_norm_'s returns, formatted)
                    state["ii"] = ii + 1
        elif route in ("fit", "fit_ema"):
            log = StepLog(fit.LOG_NAMES, read_every, c["steps_per_epoch"], dev)
            avg = WeightEMA(net, decay=ema_decay) if route == "fit_ema" else None

            def run(calls, net=net, opt=opt, rng=rng, state=state, log=log, avg=avg):
                for _ in range(calls):
                    ii = state["ii"]
                    fit.train_step(net, opt, pool, c, rng, 0, ii, alpha0, False, log)
                    if avg is not None:
                        avg.update()
                    if (ii + 1) % read_every == 0:
                        state["rows"] = log.read()
                    state["ii"] = ii + 1
        else:
            x = synth_images(batch, 3, c["patch_size"], c["patch_size"], seed=20240916).to(dev)
            gt = synth_images(batch, 3, c["patch_size"], c["patch_size"], seed=7).to(dev)
            beta0 = alpha0 * (0.02 + 0.25 * synth_images(batch, 1, c["patch_size"], c["patch_size"], seed=11).to(dev)) ** 2

            def run(calls, net=net, x=x, gt=gt, beta0=beta0):
                for _ in range(calls):
                    for p in net.parameters():
                        p.grad = None
                    mu, sig = net(x)
                    elbo_denoising_simple(mu, sig, x, gt, 1e-6, alpha0, beta0)[0].backward()
        runs[route] = run
    return runs


def _ab(runs, batch, repeats, calls, warmup):
    import torch
    for run in runs.values():
        run(warmup)
    torch.cuda.synchronize()
    rate = {name: [] for name in runs}
    for _ in range(repeats):
        for name, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(calls)
            torch.cuda.synchronize()
            rate[name].append(batch * calls / (time.perf_counter() - t0))
    return rate


def _print_row(row, rate, base, batch=None):
    """print `row` with the routes' rates: per route the median and range (and, given `batch`, the ms per step), then `fit` against `base`"""
    for name, v in rate.items():
        row[f"images_per_s_{name}"] = round(statistics.median(v), 1)
        row[f"images_per_s_{name}_range"] = [round(min(v), 1), round(max(v), 1)]
        if batch is not None:
            row[f"ms_per_step_{name}"] = round(1e3 * batch / statistics.median(v), 2)
    a, b = rate[base], rate["fit"]
    row[f"spread_{base}"] = round((max(a) - min(a)) / statistics.median(a), 4)
    row[f"fit_over_{base}"] = round(statistics.median(b) / statistics.median(a), 4)
    row["fit_not_slower"] = bool(statistics.median(b) >= statistics.median(a) * (1.0 - row[f"spread_{base}"]))
    print(json.dumps(row), flush=True)


def measure(batch, repeats, calls, read_every, dtype, ema_decay=None):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    which = ("readme", "fit", "bench_train") + (("fit_ema",) if ema_decay else ())
    rate = _ab(_routes(dev, batch, read_every, which, ema_decay), batch, repeats, calls, warmup=max(5, read_every // 10))
    row = {"row": "trainloop", "shape": [batch, 3, CFG["patch_size"], CFG["patch_size"]], "dtype": dtype, "calls_per_block": calls,
           "blocks": repeats, "log_read_every": read_every}
    if ema_decay:
        ms = {name: 1e3 * batch / statistics.median(rate[name]) for name in ("fit", "fit_ema")}
        row.update(ema_decay=ema_decay, ms_per_step_fit=round(ms["fit"], 3), ms_per_step_fit_ema=round(ms["fit_ema"], 3),
                   ema_added_ms_per_step=round(ms["fit_ema"] - ms["fit"], 3))
    _print_row(row, rate, "readme")


def launches(route):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    runs = _routes(dev, 16, 100, which=() if route == "none" else (route,))
    n = 0
    for run in runs.values():
        run(3)
        torch.cuda.synchronize()
        run(10)
        n += 10
    torch.cuda.synchronize()
    print(json.dumps({"row": "launches", "route": route, "warmup_steps": 3 if n else 0, "steps": n, "traced_steps": n + 3 if n else 0}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100, help="steps per timed block")
    ap.add_argument("--read-every", type=int, default=100, help="steps between two reads of the fit route's log (the config's print_freq)")
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"], help="conv operand form of the training step, as bench.py --dtype")
    ap.add_argument("--launches", default=None, choices=["none", "readme", "fit", "bench_train"])
    ap.add_argument("--ema-decay", type=float, default=None, metavar="X", help="also time the fit route with a weight average of decay X (route fit_ema)")
    args = ap.parse_args()
    if args.dtype == "bf16":
        os.environ["VIRNET_CONV_FORM"] = "bf16"          # (process state, read when the convs are first planned: set before any import)
    import torch
    assert torch.cuda.is_available(), "bench_trainloop needs a ROCm device"
    if args.launches:
        launches(args.launches)
        return
    for batch in args.batches:
        measure(batch, args.repeats, args.calls, args.read_every, args.dtype, args.ema_decay)


if __name__ == "__main__":
    main()
