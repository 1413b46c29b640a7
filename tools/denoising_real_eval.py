#!/usr/bin/env python
"""Counterpart of the reference's scripts/denoising_virnet_real_sidd.py and scripts/denoising_virnet_real_dnd.py on the MI355X path: the
real-noise model over the SIDD blocks (validation: PSNR / SSIM; --test: the benchmark blocks, results only) and over the DND boxes.

Restated, not copied.  What makes the results comparable with the reference's:
  * the network of both scripts (sigma_chn=3, n_feat=[96,160,224,288], dep_S=8), `module.`-prefixed checkpoints;
  * --flip (default True): the 8-way self-ensemble, here on the device (virnet_amd/ensemble.py): SIDD adds the eight back-transformed
    restorations one after the other in float32, DND takes numpy's mean over the stacked eight; uint8 blocks enter as float32(u / 255.0);
  * SIDD output = img_as_ubyte(clip(.)) saved as `denoised_res` in sidd_{val,test}_{flip,noflip}.mat; PSNR / SSIM on uint8 RGB, border 0,
    averaged over the blocks (virnet_amd/real_eval.py; the metrics run on the device, virnet_amd/metrics.py);
  * DND output = the clipped float32 box saved as `Idenoised_crop` in dnd_{flip,noflip}/%04d_%02d.mat.
Not reproduced: the scripts' timing (`megatime`), the thop FLOP print, and DND's bundle_submissions step.

The SIDD .mat files are read with scipy.io.  DND's info.mat and images are HDF5: that branch needs h5py, imports it only when --dnd_dir is
given, and is NOT tested: the suite has neither h5py nor DND files (tests cover real_eval.dnd_box, which it calls per box).

Without --ckpt_path the deterministic synthetic weights are used: the numbers are then a plumbing check.  Needs a ROCm device.

    python tools/denoising_real_eval.py --sidd_dir /data/SIDD [--test] [--flip False] [--ckpt_path virnet_denoising_real.pth]
    python tools/denoising_real_eval.py --dnd_dir /data/DND --save_dir results_dnd
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virnet_amd import real_eval  # noqa: E402

CFG = dict(im_chn=3, sigma_chn=3, n_feat=[96, 160, 224, 288], dep_S=8, n_resblocks=3, noise_cond=True, extra_mode="Input",
           noise_avg=False)        # scripts/denoising_virnet_real_sidd.py:76-83


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def load_state(ckpt_path, shapes, ema=False):
    if ckpt_path:
        sd = torch.load(ckpt_path, map_location="cpu")
        if ema or "model_state_dict" in sd:          # a training checkpoint (a bare state dict passes as it is)
            from virnet_amd import fit
            sd = fit.model_state_of(sd, ema=ema)
        return {(k[7:] if k.startswith("module.") else k): v.float() for k, v in sd.items()}
    from virnet_amd.utils.synth import synth_state_dict
    print("no --ckpt_path: deterministic synthetic weights (the numbers below are a plumbing check, not restoration quality)")
    return synth_state_dict(shapes)


def run_sidd(net, args):
    import scipy.io as sio
    if args.test:
        noisy = sio.loadmat(os.path.join(args.sidd_dir, "BenchmarkNoisyBlocksSrgb.mat"))["BenchmarkNoisyBlocksSrgb"]
        gt = None
    else:
        noisy = sio.loadmat(os.path.join(args.sidd_dir, "ValidationNoisyBlocksSrgb.mat"))["ValidationNoisyBlocksSrgb"]
        gt = sio.loadmat(os.path.join(args.sidd_dir, "ValidationGtBlocksSrgb.mat"))["ValidationGtBlocksSrgb"]
    res = real_eval.sidd_blocks(net, noisy, gt, flip=args.flip, batch=args.batch)
    if gt is not None:
        print(f"PSNR={res['psnr_mean']:.4f}, SSIM={res['ssim_mean']:.4f}", flush=True)
    if args.save_dir:
        os.makedirs(args.save_dir, exist_ok=True)
        name = f"sidd_{'test' if args.test else 'val'}_{'flip' if args.flip else 'noflip'}.mat"
        sio.savemat(os.path.join(args.save_dir, name), {"denoised_res": res["denoised"]})
        print("saved", os.path.join(args.save_dir, name))


def need_h5py():
    try:
        import h5py
    except ImportError as e:
        raise SystemExit("--dnd_dir: the DND files (info.mat, images_srgb/*.mat) are HDF5 and need the h5py package, which is not "
                         "installed") from e
    return h5py


def run_dnd(net, args):
    """dnd_submission_py/dnd_denoise.py:78-123 (denoise_srgb) around real_eval.dnd_box.  Untested: see the module docstring."""
    h5py = need_h5py()
    import scipy.io as sio
    out_folder = os.path.join(args.save_dir or "results_dnd", f"dnd_{'flip' if args.flip else 'noflip'}")
    os.makedirs(out_folder, exist_ok=True)
    with h5py.File(os.path.join(args.dnd_dir, "info.mat"), "r") as infos:
        info = infos["info"]
        bb = info["boundingboxes"]
        for i in range(50):
            with h5py.File(os.path.join(args.dnd_dir, "images_srgb", "%04d.mat" % (i + 1)), "r") as img:
                noisy = np.float32(np.array(img["InoisySRGB"]).T)
            boxes = np.array(info[bb[0][i]]).T
            for k in range(20):
                y0, y1, x0, x1 = int(boxes[k, 0] - 1), int(boxes[k, 2]), int(boxes[k, 1] - 1), int(boxes[k, 3])
                den = real_eval.dnd_box(net, noisy[y0:y1, x0:x1, :].copy(), flip=args.flip)
                sio.savemat(os.path.join(out_folder, "%04d_%02d.mat" % (i + 1, k + 1)), {"Idenoised_crop": np.float32(den)})
            print(f"[{i + 1}/50] done", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt_path", default="")
    ap.add_argument("--ema", action="store_true", help="load the checkpoint's averaged weights ('ema_state_dict', written by a training run with ema_decay) instead of the last iterate")
    ap.add_argument("--sidd_dir", default="", help="folder with the SIDD Validation*/Benchmark* .mat block files")
    ap.add_argument("--dnd_dir", default="", help="folder with the DND info.mat and images_srgb/ (needs h5py)")
    ap.add_argument("--flip", default=True, type=str2bool, help="8-way self-ensemble (default: True)")
    ap.add_argument("--test", action="store_true", help="SIDD: the benchmark blocks (no ground truth) instead of the validation blocks")
    ap.add_argument("--save_dir", default="", help="where the result .mat files go (SIDD: nothing is saved without it)")
    ap.add_argument("--batch", type=int, default=8, help="most images in one forward (8 = the orientations of one block)")
    ap.add_argument("--conv-form", default=None, choices=["wx4", "wx4x1", "f16x3", "bf16", "wino", "direct"], help="conv form for this run (ops.forward_scope(form=...), not the environment): wx4x1 = one fp16 product per Winograd position product, reduced precision, faster (INTEGRATION.md); default: VIRNET_CONV_FORM / wx4")
    args = ap.parse_args()
    if not args.sidd_dir and not args.dnd_dir:
        ap.error("give --sidd_dir and / or --dnd_dir")
    if args.dnd_dir:
        need_h5py()                                     # before any device work
    from virnet_amd import ops
    with ops.forward_scope(form=args.conv_form):
        run(args)


def run(args):
    from virnet_amd.networks import VIRAttResUNet
    net = VIRAttResUNet(**CFG)
    net.load_state_dict(load_state(args.ckpt_path, {k: tuple(v.shape) for k, v in net.state_dict().items()}, args.ema), strict=True)
    net = net.cuda().eval()
    if args.sidd_dir:
        run_sidd(net, args)
    if args.dnd_dir:
        run_dnd(net, args)


if __name__ == "__main__":
    main()
