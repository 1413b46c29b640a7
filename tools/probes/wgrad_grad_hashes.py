#!/usr/bin/env python
"""sha256 of every parameter gradient of one seeded fused denoiser step and one seeded SISR step on the test suite's small networks, under the
default conv form and VIRNET_CONV_FORM=bf16, plus the number of LaunchTimer records the step leaves: one JSON line per (step, form).
Two trees compute the same thing exactly when their lines are equal:

    python tools/probes/wgrad_grad_hashes.py [--tree OTHER_TREE] [--out FILE]

--tree imports `virnet_amd` from another checkout (with its own built library) instead of this one."""
import argparse
import hashlib
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, os.pardir))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402
from virnet_amd import ops  # noqa: E402
from virnet_amd.loss import elbo_denoising_simple  # noqa: E402
from virnet_amd.networks import VIRAttResUNet, VIRAttResUNetSR  # noqa: E402
from virnet_amd.utils.synth import synth_images, synth_state_dict  # noqa: E402

assert os.path.abspath(ops.__file__).startswith(os.path.abspath(args.tree)), ops.__file__
DENOISE = dict(im_chn=1, sigma_chn=1, n_feat=[64, 128], dep_S=3, n_resblocks=1, noise_cond=False, extra_mode="Null")
SISR = dict(im_chn=3, sigma_chn=1, kernel_chn=3, n_feat=[64, 96], dep_S=3, dep_K=2, noise_cond=True, kernel_cond=True, n_resblocks=1,
            extra_mode="Both", noise_avg=True)


def build(cls, cfg):
    net = cls(**cfg)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=5), strict=True)
    return net.cuda().train()


def denoise_loss(net):
    n, c, h, w = 2, 1, 18, 22
    gt = synth_images(n, c, h, w, seed=1).cuda()
    sig_gt = (0.02 + 0.25 * synth_images(n, 1, h, w, seed=2).cuda()) ** 2
    noisy = gt + (synth_images(n, c, h, w, seed=3).cuda() - 0.5) * 0.4
    mu, sigma = net(noisy)
    alpha0 = torch.tensor([0.5 * 7 ** 2], dtype=mu.dtype, device=mu.device)
    return elbo_denoising_simple(mu, sigma, noisy, gt, 1e-2, alpha0, alpha0 * sig_gt)[0]


def sisr_loss(net):
    # (20 x 24: KNet's stride-4 maps keep 5 rows, so its 3x3 layers too run the f16-pipe weight gradient, whose summation order is fixed; at
    #  fewer rows they run the fp32 kernel, which adds its split-K partials with atomics and differs run to run on ONE tree)
    x, gt = synth_images(2, 3, 20, 24).cuda(), synth_images(2, 3, 40, 48, seed=2).cuda()
    mu, kinfo, sigma = net(x, 2)
    return ((mu - gt) ** 2).mean() * 50 + (kinfo[:, :2].log() ** 2).mean() + (kinfo[:, 2] ** 2).mean() * 3 + (sigma.log() ** 2).mean() * 0.01


lines = []
for form in ("default", "bf16"):
    os.environ.pop("VIRNET_CONV_FORM", None)
    if form != "default":
        os.environ["VIRNET_CONV_FORM"] = form
    for step, cls, cfg, loss in (("denoise", VIRAttResUNet, DENOISE, denoise_loss), ("sisr", VIRAttResUNetSR, SISR, sisr_loss)):
        net = build(cls, cfg)
        loss(net).backward()                                 # warm-up: packings, workspaces
        for p in net.parameters():
            p.grad = None
        timer = ops.LaunchTimer()
        ops.set_launch_timer(timer)
        loss(net).backward()
        torch.cuda.synchronize()
        ops.set_launch_timer(None)
        hashes = {k: hashlib.sha256(p.grad.cpu().numpy().tobytes()).hexdigest()[:16] for k, p in net.named_parameters()}
        lines.append(json.dumps(dict(step=step, form=form, records=len(timer.records), hashes=hashes), sort_keys=True))
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
