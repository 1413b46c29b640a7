#!/usr/bin/env python
"""Time of the device SISR objective (virnet_amd/elbo.py ``elbo_sisr``) from device events, next to the torch route it can replace
(``loss.elbo_sisr``, the default), in one process:

  * ``isolated``: objective + backward with ``mu``, ``sigma_est`` and ``kinfo_est`` as leaves at 16 x 3 x 256 x 256, k = 21, sf = 4, for
    Bicubic and Direct and for each ``degrade_impl``: ``loss.elbo_sisr(impl="hip")`` against ``impl="torch"``;
  * ``train_step``: the ``bench.py --task train_sisr`` step (forward x4, objective, backward through the HIP kernels; bench.py's network, data
    and constants) with the keyword switched, for each ``degrade_impl``.

Every figure is the median of ``--repeats`` timed blocks of ``--calls`` calls after warm-up, with the minimum and the maximum of the blocks
beside it; the two routes alternate block by block.  The torch route is the code of the parent commit, unchanged.  Prints one JSON line per row.

    python tools/bench_elbo_sisr.py [--repeats 15] [--calls 20] [--step-calls 5] [--dtype f32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_elbo import _ab, _put  # noqa: E402

CONSTS = dict(r2=1e-4, eps2=1e-5, sf=4, k_size=21, penalty_K=[0.02, 2], shift=False)


def isolated(repeats, calls):
    import torch
    from virnet_amd import loss
    n, c, lr, sf = 16, 3, 64, 4
    g = torch.Generator().manual_seed(1)
    hr = lr * sf
    im_hr, im_lr = torch.rand(n, c, hr, hr, generator=g).cuda(), torch.rand(n, c, lr, lr, generator=g).cuda()
    mu = (im_hr + 0.01 * torch.randn(n, c, hr, hr, generator=g).cuda()).requires_grad_(True)
    sigma = (torch.rand(n, 1, 1, 1, generator=g) * 0.01 + 1e-4).cuda().requires_grad_(True)
    kinfo = torch.cat([torch.rand(n, 2, generator=g) * 3 + 0.5, torch.rand(n, 1, generator=g) * 1.2 - 0.6], 1).cuda().requires_grad_(True)
    kinfo_gt = torch.tensor([[1.2, 0.8, 0.1]], device="cuda").repeat(n, 1)
    nlevel = torch.empty((n, 1, 1, 1), device="cuda").fill_(2e-3)
    alpha0, kappa0 = 0.5 * torch.tensor([9.0 ** 2], device="cuda"), torch.tensor([50.0], device="cuda")
    for down in ("Bicubic", "Direct"):
        for degrade_impl in ("torch", "hip"):
            def both(impl):
                out = loss.elbo_sisr(mu=mu, sigma_est=sigma, kinfo_est=kinfo, im_hr=im_hr, im_lr=im_lr, sigma_prior=nlevel, alpha0=alpha0, kinfo_gt=kinfo_gt,
                                     kappa0=kappa0, downsampler=down, degrade_impl=degrade_impl, impl=impl, **CONSTS)[0]
                return out, torch.autograd.grad(out, [mu, sigma, kinfo])

            def seeded(impl):
                torch.manual_seed(3)
                return both(impl)
            (oh, gh), (ot, gt_) = seeded("hip"), seeded("torch")
            row = {"row": "isolated", "shape": [n, c, hr, hr], "k": 21, "sf": sf, "downsampler": down, "degrade_impl": degrade_impl,
                   "calls_per_block": calls, "blocks": repeats, "loss_hip": float(oh.detach()), "loss_torch": float(ot.detach())}
            for name, a, b in zip(("dmu", "dsigma", "dkinfo"), gh, gt_):
                row[f"{name}_max_rel_diff"] = float((a - b).abs().max() / b.abs().max())
            _put(row, "loss_and_backward", _ab({"hip": lambda: both("hip"), "torch": lambda: both("torch")}, repeats, calls))
            print(json.dumps(row), flush=True)


def train_step(repeats, calls, dtype):
    import torch
    import bench
    from virnet_amd.loss import elbo_sisr
    from virnet_amd.utils.synth import synth_images
    dev = torch.device("cuda", torch.cuda.current_device())
    net, sd = bench.build_net(dev, "sisr")
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    n, size = 16, 64
    x = synth_images(n, 3, size, size, seed=20240916).to(dev)
    im_hr = synth_images(n, 3, size * 4, size * 4, seed=7).to(dev)
    kinfo_gt = torch.tensor([[1.2, 0.8, 0.1]], device=dev).repeat(n, 1)
    nlevel = torch.empty((n, 1, 1, 1), device=dev).fill_(2e-3)
    alpha0, kappa0 = 0.5 * torch.tensor([9.0 ** 2], device=dev), torch.tensor([50.0], device=dev)
    for degrade_impl in ("torch", "hip"):
        def step(impl):
            for p in net.parameters():
                p.grad = None
            mu, kinfo, sig = net(x, 4)
            out = elbo_sisr(mu=mu, sigma_est=sig, kinfo_est=kinfo, im_hr=im_hr, im_lr=x, sigma_prior=nlevel, alpha0=alpha0, kinfo_gt=kinfo_gt, kappa0=kappa0,
                            downsampler="Bicubic", degrade_impl=degrade_impl, impl=impl, **CONSTS)[0]
            out.backward()
            return out.detach()

        def seeded(impl):
            torch.manual_seed(3)
            return float(step(impl))
        lh, lt = seeded("hip"), seeded("torch")
        row = {"row": "train_step", "shape": [n, 3, size, size], "dtype": dtype, "downsampler": "Bicubic", "degrade_impl": degrade_impl,
               "calls_per_block": calls, "blocks": repeats, "loss_hip": lh, "loss_torch": lt}
        _put(row, "step", _ab({"hip": lambda: step("hip"), "torch": lambda: step("torch")}, repeats, calls, warmup=3))
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--step-calls", type=int, default=5, help="training steps per timed block")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="conv operand form of the training step, as bench.py --dtype (its default: f32)")
    ap.add_argument("--skip-train", action="store_true", help="only the isolated rows")
    args = ap.parse_args()
    if args.dtype == "bf16":
        os.environ["VIRNET_CONV_FORM"] = "bf16"          # (process state, read when the convs are first planned: set before any import)
    import torch
    assert torch.cuda.is_available(), "bench_elbo_sisr needs a ROCm device"
    isolated(args.repeats, args.calls)
    if not args.skip_train:
        train_step(args.repeats, args.step_calls, args.dtype)


if __name__ == "__main__":
    main()
