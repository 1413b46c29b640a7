#!/usr/bin/env python
"""Counterpart of the reference's train_SISR.py on the MI355X path (same flags: --config --save_dir, and --resume, which the reference
reads from the config).

Restated, not copied: reads the reference's config file as it is (JSON with ``#`` comments, configs/sisr_x2.json / sisr_x3.json /
sisr_x4.json; the booleans are the strings "True" / "False"), decodes ``train_hr_patchs/*.png`` with PIL into ONE device-resident uint8 pool,
builds the network as train_SISR.py:78-87 does (the reference's seed; ``noise_avg = not add_jpeg``), builds one
``datagen.GeneralTestSet`` per noise type ("Gaussian", and "JPEG" with ``add_jpeg``) over ``val_hr_path/*.bmp`` -- every validation
image is degraded once and stays on the device -- and calls ``virnet_amd.fit.fit_sisr``: batches, objective, clipping, Adam, the step log
and the validation stay on the device, and the host reads it once per ``print_freq`` steps.  Without validation images the test stage is
skipped.  Two more optional config keys: ``steps_per_epoch`` (default 10000, the reference's dataset length over its batch size) and
``max_images`` (decode at most that many training patches).  TensorBoard summaries are not reproduced.  ``--gpus N`` (or torchrun) trains
data-parallel as the reference's one process per device does: ``batch_size`` is the global batch, every rank builds its own pool, rank 0
prints, validates and saves.  ``--ema-decay X [--ema-warmup]`` (or the config keys ``ema_decay`` / ``ema_warmup``; the flags win) keeps an
exponential moving average of the weights on the device, validates on it and saves it as ``ema_state_dict``.

    python tools/train_sisr.py --config configs/sisr_x4.json --save_dir train_save [--resume train_save/models/model_3.pth] [--gpus 8]
        [--ema-decay 0.999 [--ema-warmup]]
"""
import os
import sys
from pathlib import Path

import train_common as tc          # (the sibling module; importing it puts the repository root on sys.path)


def build_net(args: dict, device):
    import torch
    from virnet_amd import fit
    from virnet_amd.networks import VIRAttResUNetSR
    torch.manual_seed(1234)          # train_SISR.py:74-75: the seed before the network is initialised
    torch.cuda.manual_seed_all(1234)
    net = VIRAttResUNetSR(im_chn=args["im_chn"], sigma_chn=args["sigma_chn"], dep_K=args["dep_K"], dep_S=args["dep_S"], n_feat=args["n_feat"],
                          n_resblocks=args["n_resblocks"], noise_cond=fit.str2bool(args["noise_cond"], "noise_cond"),
                          kernel_cond=fit.str2bool(args["kernel_cond"], "kernel_cond"), extra_mode=args["extra_mode"],
                          noise_avg=not fit.str2bool(args["add_jpeg"], "add_jpeg"))
    return net.to(device)


def main():
    args = tc.read_args("./configs/sisr_x4.json", "./train_save", "Path to save the log file", 20, config_first=True)
    from virnet_amd import datagen, fit
    c = fit.read_sisr_config(args)
    device = tc.device("train_sisr")
    net = build_net(args, device)
    tc.print_parameter_counts(net, ("SNet", "KNet", "RNet"))
    files = sorted(str(x) for x in Path(args["train_hr_patchs"]).glob("*.png"))
    if args.get("max_images"):
        files = files[:int(args["max_images"])]
    if not files:
        sys.exit("no training images: point train_hr_patchs of the config at the folder of HR patches (*.png)")
    pool = datagen.ImagePool(tc.read_images(files, c["hr_size"], "train"), device)
    print(f"Number of Patches in training data set: {len(pool):d}", flush=True)
    val = None
    val_files = sorted(str(x) for x in Path(args.get("val_hr_path", os.path.join("test_data", "Set14"))).glob("*.bmp"))
    if val_files:
        val_pool = datagen.ImagePool(tc.read_images(val_files, 11 + 2 * c["sf"] ** 2 + c["sf"], "test"), device)
        val = {x: datagen.GeneralTestSet(val_pool, c["sf"], c["k_size"], c["kernel_shift"], c["downsampler"], x)
               for x in ["Gaussian"] + (["JPEG"] if c["add_jpeg"] else [])}
    else:
        print("no validation images found: the test stage is skipped", flush=True)
    print(f"T_max = {c['epochs']:d}, eta_min={c['lr_min']:.2e}")
    fit.fit_sisr(net, pool, args, val=val, save_dir=args["save_dir"], resume=tc.resume_path(args), log=lambda s: print(s, flush=True),
                 writer=tc.summary_writer(args))


if __name__ == "__main__":
    main()
