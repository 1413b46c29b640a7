#!/usr/bin/env python
"""Counterpart of the reference's train_denoising_real.py on the MI355X path (same flags: --config --save_dir, and --resume, which the
reference reads from the config).

Restated, not copied: reads the reference's config file as it is (JSON with ``#`` comments, configs/denoising_real.json), loads the paired
training patches into ONE device-resident paired uint8 pool, builds the network from the config with the reference's seed, and calls
``virnet_amd.fit.fit_denoising(..., real=True)``: paired crops, MixUp, the variance prior, the objective, clipping, Adam and the step log
stay on the device.

Data, as folders or ``.npy`` arrays of paired uint8 images (LMDB and H5 readers stay with the caller):
  * ``train_pch_dir``: the folder of noisy PNG patches; the ground truth of ``<dir>/x.png`` is ``<dir>/../gt/x.png`` (RealTrain,
    datasets/DenoisingDatasets.py:114-129; of its stem filter only ``sidd`` is on in the reference's call, and it is applied when any file
    matches it) -- or a ``.npy`` array [M,H,W,3] of noisy patches, with ``train_gt`` naming the array of ground truths;
  * ``test_noisy_path`` / ``test_gt_path``: ``.npy`` arrays [..., H, W, 3] of equal-size validation blocks (the SIDD validation ``.mat``
    arrays saved with numpy), or two folders of PNG blocks with equal file names; absent or not found: the test stage is skipped.
``lr_min`` defaults to the script's hard-coded 1e-6; ``steps_per_epoch`` (default 10000) and ``max_images`` are optional keys.  ``--gpus N``
(or torchrun) trains data-parallel: ``batch_size`` is the global batch, MixUp pairs rows of the WHOLE batch (a row's partner may be
synthesised on another rank as well), every rank builds its own pool, rank 0 prints, validates and saves.  ``--ema-decay X
[--ema-warmup]`` (or the config keys ``ema_decay`` / ``ema_warmup``; the flags win) keeps an exponential moving average of the weights on
the device, validates on it and saves it as ``ema_state_dict``.

    python tools/train_denoising_real.py --config configs/denoising_real.json --save_dir train_record [--gpus 8] [--ema-decay 0.999 [--ema-warmup]]
"""
import os
import sys
from pathlib import Path

import numpy as np

import train_common as tc          # (the sibling module; importing it puts the repository root on sys.path)
from train_denoising_syn import build_net          # (the sibling driver: same network construction)


def load_pairs(noisy_src, gt_src, limit=None, smallest=1, what="train"):
    """(noisy, gt): two lists of uint8 [H,W,3] arrays from two ``.npy`` arrays or from a folder of noisy PNGs (and its ``gt`` sibling, or
    the folder ``gt_src``)."""
    if str(noisy_src).endswith(".npy"):
        noisy, gt = np.load(noisy_src), np.load(gt_src)
        if noisy.shape != gt.shape or noisy.dtype != np.uint8 or gt.dtype != np.uint8 or noisy.shape[-1] != 3:
            sys.exit(f"{what}: {noisy_src} {noisy.shape} {noisy.dtype} and {gt_src} {gt.shape} {gt.dtype}: two uint8 arrays [...,H,W,3] of one shape are expected")
        noisy, gt = noisy.reshape((-1,) + noisy.shape[-3:]), gt.reshape((-1,) + gt.shape[-3:])
        return list(noisy[:limit]), list(gt[:limit])
    files = sorted(Path(noisy_src).glob("*.png"))
    if gt_src is None and any("sidd" in f.stem for f in files):
        files = [f for f in files if "sidd" in f.stem]
    files = files[:limit]
    gt_files = [(Path(gt_src) if gt_src else f.parents[1] / "gt") / f.name for f in files]
    return tc.read_images(files, smallest, what), tc.read_images(gt_files, smallest, what)


def main():
    args = tc.read_args("./configs/denoising_real.json", "./train_record", "Path to save the model and log file", 15)
    from virnet_amd import datagen, fit
    device = tc.device("train_denoising_real")
    net = build_net(args, device)
    tc.print_parameter_counts(net, ("SNet", "RNet"))
    limit = int(args["max_images"]) if args.get("max_images") else None
    noisy, gt = load_pairs(args["train_pch_dir"], args.get("train_gt"), limit, int(args["patch_size"]))
    if not noisy or len(noisy) != len(gt):
        sys.exit(f"{len(noisy)} noisy and {len(gt)} ground-truth training patches: point train_pch_dir (and train_gt) of the config at the data")
    print(f"Number of Patches in training data set: {len(noisy):d}", flush=True)
    pool = datagen.ImagePool.paired(noisy, gt, device)
    val = None
    tn, tg = args.get("test_noisy_path"), args.get("test_gt_path")
    if tn and tg and os.path.exists(tn) and os.path.exists(tg) and (str(tn).endswith(".npy") or os.path.isdir(tn)):
        vn, vg = load_pairs(tn, tg, None, 11, "test")
        val = datagen.ImagePool.paired(vn, vg, device) if vn else None
    if val is None:
        print("no validation blocks found (.npy arrays or PNG folders): the test stage is skipped", flush=True)
    args.setdefault("lr_min", 1e-6)          # train_denoising_real.py:75: hard-coded there
    print(f"T_max = {args['epochs'] - args['warmup_epochs']:d}, eta_min={args['lr_min']:.2e}")
    fit.fit_denoising(net, pool, args, val=val, real=True, save_dir=args["save_dir"], resume=tc.resume_path(args), log=lambda s: print(s, flush=True),
                      writer=tc.summary_writer(args))


if __name__ == "__main__":
    main()
