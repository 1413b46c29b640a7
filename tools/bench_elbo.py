#!/usr/bin/env python
"""Time of the device objective (virnet_amd/elbo.py) from device events, next to the torch routes it can replace, in one process:

  * ``isolated``: loss + backward with ``mu`` and ``sigma_est`` as leaves at 32 x 3 x 256 x 256, sigma_est / beta0 with one channel and with
    three: ``loss.elbo_denoising_simple(impl="hip")`` against ``impl="torch"`` (the default);
  * ``noise_estimate``: ``elbo.noise_estimate`` against the reference's form on the device, reflect pad + grouped ``F.conv2d`` of the squared
    error + clamp (utils/util_denoising.py:42-63), k = 7, same shape;
  * ``train_step``: the ``bench.py --task train`` step (forward, objective, backward through the HIP kernels; bench.py's network, data and
    prior) with the keyword switched, at each of ``--sizes`` (bench.py's training patch is 128).

Every figure is the median of ``--repeats`` timed blocks of ``--calls`` calls after warm-up, with the minimum and the maximum of the blocks
beside it; the two implementations alternate block by block.  Prints one JSON line per row.

    python tools/bench_elbo.py [--repeats 15] [--calls 20] [--dtype bf16] [--sizes 128 256]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _block_ms(step, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def _ab(steps, repeats, calls, warmup=5):
    """{name: (median ms per call, min, max)} with the implementations alternating block by block"""
    import torch
    for step in steps.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    ms = {name: [] for name in steps}
    for _ in range(repeats):
        for name, step in steps.items():
            ms[name].append(_block_ms(step, calls))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def _put(row, what, res):
    for impl, (med, lo, hi) in res.items():
        row[f"{what}_ms_{impl}"] = round(med, 4)
        row[f"{what}_ms_{impl}_range"] = [round(lo, 4), round(hi, 4)]


def isolated(repeats, calls):
    import torch
    from virnet_amd import loss
    n, c, hw = 32, 3, 256
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(n, c, hw, hw, generator=g).cuda()
    alpha0 = torch.tensor([24.5], device="cuda")
    for chn in (1, 3):
        var = ((0.02 + 0.25 * torch.rand(n, chn, hw, hw, generator=g)) ** 2).cuda()
        noisy = gt + var.sqrt() * torch.randn(n, c, hw, hw, generator=g).cuda()
        mu = (gt + 0.01 * torch.randn(n, c, hw, hw, generator=g).cuda()).requires_grad_(True)
        sigma = (var * torch.exp(0.3 * torch.randn(n, chn, hw, hw, generator=g).cuda())).requires_grad_(True)
        beta0 = alpha0 * var

        def both(impl):
            out = loss.elbo_denoising_simple(mu, sigma, noisy, gt, 1e-6, alpha0, beta0, impl=impl)
            return out, torch.autograd.grad(out[0], [mu, sigma])

        (oh, gh), (ot, gt_) = both("hip"), both("torch")
        row = {"row": "isolated", "shape": [n, c, hw, hw], "sigma_channels": chn, "beta0_channels": chn, "calls_per_block": calls, "blocks": repeats,
               "loss_hip": float(oh[0].detach()), "loss_torch": float(ot[0].detach()),
               "dmu_max_rel_diff": float((gh[0] - gt_[0]).abs().max() / gt_[0].abs().max()),
               "dsigma_max_rel_diff": float((gh[1] - gt_[1]).abs().max() / gt_[1].abs().max())}
        _put(row, "loss_and_backward", _ab({"hip": lambda: both("hip"), "torch": lambda: both("torch")}, repeats, calls))
        print(json.dumps(row), flush=True)


def noise_estimate(repeats, calls):
    import torch
    import torch.nn.functional as F
    from virnet_amd import elbo
    n, c, hw, k = 32, 3, 256, 7
    g = torch.Generator().manual_seed(2)
    gt = torch.rand(n, c, hw, hw, generator=g).cuda()
    noisy = gt + 0.1 * torch.randn(n, c, hw, hw, generator=g).cuda()
    g1 = torch.from_numpy(elbo.gaussian_taps(k))
    k2 = (g1[:, None] * g1[None, :])
    kernel = (k2 / k2.sum()).float().expand(c, 1, k, k).contiguous().cuda()

    def torch_form():
        out = F.conv2d(F.pad((noisy - gt) ** 2, (k // 2,) * 4, mode="reflect"), kernel, groups=c)
        return out.clamp_(min=1e-10)

    def hip_form():
        return elbo.noise_estimate(noisy, gt, k)

    a, b = hip_form(), torch_form()
    row = {"row": "noise_estimate", "shape": [n, c, hw, hw], "k": k, "calls_per_block": calls, "blocks": repeats,
           "max_rel_diff": float(((a - b).abs() / b).max())}
    _put(row, "call", _ab({"hip": hip_form, "torch": torch_form}, repeats, calls))
    print(json.dumps(row), flush=True)


def train_step(size, repeats, calls, dtype):
    import torch
    import bench
    from virnet_amd.loss import elbo_denoising_simple
    from virnet_amd.utils.synth import synth_images
    dev = torch.device("cuda", torch.cuda.current_device())
    net, sd = bench.build_net(dev, "denoise")
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    n = 32
    x = synth_images(n, 3, size, size, seed=20240916).to(dev)
    gt = synth_images(n, 3, size, size, seed=7).to(dev)
    sigma_gt = (0.02 + 0.25 * synth_images(n, 1, size, size, seed=11).to(dev)) ** 2
    alpha0 = torch.tensor([0.5 * 7 ** 2], dtype=torch.float32, device=dev)
    beta0 = alpha0 * sigma_gt
    layout = {}

    def step(impl):
        for p in net.parameters():
            p.grad = None
        mu, sig = net(x)
        layout.update(mu_contiguous=mu.is_contiguous(), sigma_contiguous=sig.is_contiguous(), sigma_shape=list(sig.shape))
        out = elbo_denoising_simple(mu, sig, x, gt, 1e-6, alpha0, beta0, impl=impl)[0]
        out.backward()
        return out.detach()

    lh, lt = float(step("hip")), float(step("torch"))
    row = {"row": "train_step", "shape": [n, 3, size, size], "dtype": dtype, "calls_per_block": calls, "blocks": repeats, "loss_hip": lh, "loss_torch": lt,
           **layout}
    _put(row, "step", _ab({"hip": lambda: step("hip"), "torch": lambda: step("torch")}, repeats, calls, warmup=3))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--step-calls", type=int, default=5, help="training steps per timed block")
    ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"], help="conv operand form of the training step, as bench.py --dtype")
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256], help="patch sizes of the train_step rows")
    args = ap.parse_args()
    if args.dtype == "bf16":
        os.environ["VIRNET_CONV_FORM"] = "bf16"          # (process state, read when the convs are first planned: set before any import)
    import torch
    assert torch.cuda.is_available(), "bench_elbo needs a ROCm device"
    isolated(args.repeats, args.calls)
    noise_estimate(args.repeats, args.calls)
    for size in args.sizes:
        train_step(size, args.repeats, args.step_calls, args.dtype)


if __name__ == "__main__":
    main()
