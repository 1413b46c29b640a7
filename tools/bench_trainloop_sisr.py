#!/usr/bin/env python
"""Images per second of the SISR training loop on the device (virnet_amd/fit.py fit_sisr), next to the loop a user writes by hand, in one
process, on bench.py's SISR network (configs/sisr_x4.json: n_feat 96/160/224, 2 res-blocks, dep_S 5, dep_K 8) at the shipped shape: batch
16, HR patches of 192 x 192, sf 4 (LR 48 x 48):

  * ``hand``: the loop body written from the package's pieces -- ``datagen.sisr_batch``, forward, ``elbo.elbo_sisr``, backward,
    ``ClipAdam.step()`` -- with the reference's eight host reads per step (train_SISR.py:232-243: five ``.item()`` calls and the three
    gradient norms);
  * ``fit``: ``fit.sisr_train_step`` -- the same launches plus the ``StepLog`` push -- with the log read once per ``--read-every`` steps.

A block is ``--calls`` steps between two device synchronisations, timed on the host clock (the host reads are the subject); the routes
alternate block by block, ``--repeats`` blocks each after warm-up.  Per route the median images/s with the minimum and the maximum of the
blocks; ``spread_hand`` is (max - min) / median of the ``hand`` blocks, the yardstick for "not slower": ``fit`` passes when its median is not
below the ``hand`` median by more than that spread.  Prints one JSON line.

``--sft-kernel`` instead times the SFT backward alone at the three shapes the shipped step runs it at (16 x 192^2 x 96, 16 x 96^2 x 160,
16 x 48^2 x 224): ``atomic`` = ``virnet_sft_backward`` (one launch; the two zero fills it needs before it are NOT in the time),
``ordered`` = ``virnet_sft_backward_ordered`` (two launches, no fill), on preallocated buffers so that the host only launches; device events
around ``--calls`` calls, the routes alternating, median of ``--repeats``.  One JSON line per shape.

    python tools/bench_trainloop_sisr.py [--repeats 5] [--calls 100]
    python tools/bench_trainloop_sisr.py --sft-kernel
"""
import argparse
import json
import random
import statistics

from bench_trainloop import _ab, _pool, _print_row          # (the denoising loop's tool: same pool, block timer and row; it puts the root on sys.path)

# configs/sisr_x4.json
CFG = dict(hr_size=192, batch_size=16, epochs=120, lr=2e-4, lr_min=1e-6, print_freq=100, sf=4, k_size=21, add_jpeg="False", kernel_shift="False",
           downsampler="Bicubic", noise_level=[0.01, 15], noise_jpeg=[0.01, 10], eps2=1e-5, r2=1e-4, var_window=9, kappa0=50, penalty_K=[0.02, 2],
           clip_grad_R=5e2, clip_grad_S=1e2, clip_grad_K=5e2, steps_per_epoch=10000)
SFT_SHAPES = [(16, 192, 192, 96), (16, 96, 96, 160), (16, 48, 48, 224)]


def _routes(dev, read_every):
    """{route: run(calls)} each over its own copy of the network; run() enqueues `calls` steps with the route's own host reads"""
    import torch
    import bench
    from virnet_amd import datagen, elbo, fit
    from virnet_amd.trainlog import StepLog
    c = fit.read_sisr_config(CFG)
    pool = _pool(dev)
    alpha0 = (0.5 * torch.tensor([c["var_window"] ** 2], dtype=torch.float32)).to(dev)
    kappa0 = torch.tensor([c["kappa0"]], dtype=torch.float32).to(dev)
    b, hr, sf = c["batch_size"], c["hr_size"], c["sf"]
    runs = {}
    for route in ("hand", "fit"):
        net, sd = bench.build_net(dev, "sisr")
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).train()
        opt = fit.sisr_optimizer(net, c)
        rng = random.Random(0)
        state = {"ii": 0, "acc": [0.0] * 5}
        if route == "hand":
            def run(calls, net=net, opt=opt, rng=rng, state=state):
                for _ in range(calls):
                    ii = state["ii"]
                    params = datagen.draw_sisr_params(rng, pool, b, hr, sf, c["noise_level"], c["add_jpeg"], c["noise_jpeg"])
                    im_hr, im_lr, im_blur, kinfo_gt, nlevel = datagen.sisr_batch(pool, params, hr, sf, c["k_size"], seed=0, downsampler=c["downsampler"],
                                                                                 shift=c["kernel_shift"], base_id=ii * b)
                    opt.zero_grad()
                    mu, kinfo_est, sigma_est = net(im_lr, sf)
                    loss, detail = elbo.elbo_sisr(mu=mu, sigma_est=sigma_est, kinfo_est=kinfo_est, im_hr=im_hr, im_lr=im_lr, sigma_prior=nlevel,
                                                  alpha0=alpha0, kinfo_gt=kinfo_gt, kappa0=kappa0, r2=c["r2"], eps2=c["eps2"], sf=sf, k_size=c["k_size"],
                                                  penalty_K=c["penalty_K"], downsampler=c["downsampler"], shift=c["kernel_shift"])
                    loss.backward()
                    opt.step()
                    for k, v in enumerate((loss, detail[0], detail[1], detail[2], detail[3])):          # train_SISR.py:232-236
                        state["acc"][k] += v.item() / c["steps_per_epoch"]
                    state["norms"] = tuple(float(opt.grad_norms[k]) for k in range(3))                    # :243 (clip_grad_norm_'s returns, formatted)
                    state["ii"] = ii + 1
        else:
            log = StepLog(fit.SISR_LOG_NAMES, read_every, c["steps_per_epoch"], dev)

            def run(calls, net=net, opt=opt, rng=rng, state=state, log=log):
                for _ in range(calls):
                    ii = state["ii"]
                    fit.sisr_train_step(net, opt, pool, c, rng, 0, ii, alpha0, kappa0, log)
                    if (ii + 1) % read_every == 0:
                        state["rows"] = log.read()
                    state["ii"] = ii + 1
        runs[route] = run
    return runs


def measure(repeats, calls, read_every):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    batch = CFG["batch_size"]
    rate = _ab(_routes(dev, read_every), batch, repeats, calls, warmup=max(5, read_every // 10))
    _print_row({"row": "trainloop_sisr", "shape": [batch, 3, CFG["hr_size"], CFG["hr_size"]], "sf": CFG["sf"], "calls_per_block": calls,
                "blocks": repeats, "log_read_every": read_every}, rate, "hand", batch)


def sft_kernel(repeats, calls):
    import torch
    from virnet_amd import _native as nat
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    for n, h, w, c in SFT_SHAPES:
        g = torch.Generator().manual_seed(c)
        da, x, res = ((torch.rand(n, h, w, c, generator=g) - 0.5).to(dev) for _ in range(3))
        mul, add = (0.3 + torch.rand(n, c, generator=g)).to(dev), (torch.rand(n, c, generator=g) - 0.5).to(dev)
        dx = torch.empty_like(x)
        part = torch.empty(lib.virnet_sft_backward_scratch_bytes(n, h * w, c) // 4, dtype=torch.float32, device=dev)
        head = (nat.ptr(da), nat.ptr(x), nat.ptr(mul), nat.ptr(add), nat.ptr(res), 0.2, nat.ptr(dx))

        dmul, dadd = torch.zeros((n, c), dtype=torch.float32, device=dev), torch.zeros((n, c), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def atomic():          # (keeps accumulating onto dmul / dadd: the values are not the subject)
            nat.check(lib.virnet_sft_backward(*head, nat.ptr(dmul), nat.ptr(dadd), n, h * w, c, st), "sft_backward")

        def ordered():
            nat.check(lib.virnet_sft_backward_ordered(*head, nat.ptr(dmul), nat.ptr(dadd), nat.ptr(part), n, h * w, c, st), "sft_backward_ordered")

        routes = {"atomic": atomic, "ordered": ordered}
        us = {k: [] for k in routes}
        for f in routes.values():
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for name, f in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    f()
                e1.record()
                e1.synchronize()
                us[name].append(1e3 * e0.elapsed_time(e1) / calls)
        row = {"row": "sft_backward", "shape": [n, h, w, c], "calls_per_block": calls, "blocks": repeats,
               "bytes_moved": 4 * n * h * w * c * 4}          # da, x, res read; dx written
        for name, v in us.items():
            row[f"us_{name}"] = round(statistics.median(v), 2)
            row[f"us_{name}_range"] = [round(min(v), 2), round(max(v), 2)]
        row["ordered_over_atomic"] = round(row["us_ordered"] / row["us_atomic"], 4)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100, help="steps (or kernel calls) per timed block")
    ap.add_argument("--read-every", type=int, default=100, help="steps between two reads of the fit route's log (the config's print_freq)")
    ap.add_argument("--sft-kernel", action="store_true", help="time the SFT backward alone, atomic against ordered, at the shipped step's three shapes")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_trainloop_sisr needs a ROCm device"
    if args.sft_kernel:
        sft_kernel(args.repeats, args.calls)
    else:
        measure(args.repeats, args.calls, args.read_every)


if __name__ == "__main__":
    main()
