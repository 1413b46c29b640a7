#!/usr/bin/env python
"""Counterpart of the reference's scripts/sisr_virnet_syn.py (BASELINE configs[3]) on the MI355X path: PSNR-Y / SSIM-Y of the SISR
model per dataset and per synthetic blur kernel (seven anisotropic Gaussians), noise level 2.55 by default.

Restated, not copied (virnet_amd/sisr_eval.py: kernels, blur, antialiased bicubic downscale, seeded noise -- pinned to the reference's
helpers by tests/golden/sisr_harness.npz).  With --lpips-weights (the `lpips` package's AlexNet weights, exported as INTEGRATION.md
says) the script's third column, LPIPS, is reported too (virnet_amd/lpips.py: on the device with --device-metrics, else the float32 torch
definition on the host).  Without --ckpt_path the deterministic synthetic weights are used: a plumbing check, not restoration quality.
Needs a ROCm device.

    python tools/sisr_syn_eval.py --sf 4 --data tests/golden/set5:bmp [--ckpt_path model_zoo/virnet_sisr_x4.pth] [--nlevel 2.55]
        [--device-degrade] [--device-metrics] [--lpips-weights lpips_alex.pt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virnet_amd import sisr_eval  # noqa: E402

# scripts/sisr_virnet_syn.py:53-63
CFG = dict(im_chn=3, sigma_chn=1, kernel_chn=3, n_feat=[96, 160, 224], dep_S=5, dep_K=8, noise_cond=True, kernel_cond=True,
           n_resblocks=2, extra_mode="Both", noise_avg=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt_path", default="")
    ap.add_argument("--ema", action="store_true", help="load the checkpoint's averaged weights ('ema_state_dict', written by a training run with ema_decay) instead of the last iterate")
    ap.add_argument("--sf", type=int, default=4)
    ap.add_argument("--nlevel", type=float, default=2.55)
    ap.add_argument("--data", nargs="+", default=["test_data/Set14:bmp", "test_data/CBSD68:png"], help="folder:extension, in script order")
    ap.add_argument("--device-metrics", action="store_true", help="PSNR-Y / SSIM-Y on the device instead of float64 numpy on the host")
    ap.add_argument("--device-degrade", action="store_true", help="blur, clip and bicubic downscale on the device (virnet_amd/degrade.py) "
                    "instead of scipy / numpy on the host; the seeded noise stays the host's stream")
    ap.add_argument("--qf", type=int, default=None, help="JPEG quality of a round trip that ends the degradation (the reference's GeneralTest "
                    "uses 40); on the device with --device-degrade.  Default: no JPEG")
    ap.add_argument("--lpips-weights", default="", help="state dict of lpips.LPIPS(net='alex') (or the flat layout of virnet_amd.lpips."
                    "load_weights): adds the LPIPS column of scripts/sisr_virnet_syn.py:158-161,169")
    ap.add_argument("--conv-form", default=None, choices=["wx4", "wx4x1", "f16x3", "bf16", "wino", "direct"], help="conv form for this run (ops.forward_scope(form=...), not the environment): wx4x1 = one fp16 product per Winograd position product, reduced precision, faster (INTEGRATION.md); default: VIRNET_CONV_FORM / wx4")
    args = ap.parse_args()
    from virnet_amd import ops
    with ops.forward_scope(form=args.conv_form):
        run(args)


def run(args):
    from virnet_amd.networks import VIRAttResUNetSR
    lpips_weights = None
    if args.lpips_weights:
        from virnet_amd import lpips
        lpips_weights = lpips.load_weights(args.lpips_weights)
    net = VIRAttResUNetSR(**CFG)
    if args.ckpt_path:
        sd = torch.load(args.ckpt_path, map_location="cpu")
        if args.ema or "model_state_dict" in sd:          # a training checkpoint (a bare state dict passes as it is)
            from virnet_amd import fit
            sd = fit.model_state_of(sd, ema=args.ema)
        sd = {(k[7:] if k.startswith("module.") else k): v.float() for k, v in sd.items()}
    else:
        from virnet_amd.utils.synth import synth_state_dict
        print("no --ckpt_path: deterministic synthetic weights (the numbers below are a plumbing check, not restoration quality)")
        sd = synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()

    def to_device(lr, sf):
        """the LR input as a CUDA tensor: an HWC array from the host degradation, or already [1,3,h,w] on the device (--device-degrade)"""
        return lr if isinstance(lr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lr.transpose(2, 0, 1)[np.newaxis])).cuda()

    def forward(lr, sf):
        with torch.no_grad():
            return net(to_device(lr, sf), sf)[0].squeeze(0).cpu().numpy().transpose(1, 2, 0)

    def forward_device(lr, sf):
        with torch.no_grad():
            return net(to_device(lr, sf), sf)[0]

    if args.device_metrics:
        rows = sisr_eval.sisr_table(forward_device, args.data, args.sf, nlevel=args.nlevel, device_metrics=True, device_degrade=args.device_degrade, qf=args.qf,
                                    lpips=lpips_weights)
    else:
        rows = sisr_eval.sisr_table(forward, args.data, args.sf, nlevel=args.nlevel, device_degrade=args.device_degrade, qf=args.qf,
                                    lpips=lpips_weights)
    if not rows:
        print("no images found under", args.data)
    for r in rows:
        tail = f", LPIPS: {r['lpips']:6.4f}" if "lpips" in r else ""
        print(f"Dataset: {r['dataset']:>8s}, Kernel: {r['kernel']:d}, PSNRY: {r['psnr_y']:5.2f}, SSIMY: {r['ssim_y']:6.4f}{tail}", flush=True)


if __name__ == "__main__":
    main()
