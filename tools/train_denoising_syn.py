#!/usr/bin/env python
"""Counterpart of the reference's train_denoising_syn.py on the MI355X path (same flags: --config --save_dir, and --resume, which the
reference reads from the config).

Restated, not copied: reads the reference's config file as it is (JSON with ``#`` comments, configs/denoising_syn.json), decodes the
training folders it names (CBSD_path *.jpg, WED_path *.bmp, Flickr *.png, DIV2K *.png; a missing folder contributes nothing) with PIL
into ONE device-resident uint8 pool, builds the network from the config with the reference's seed, and calls
``virnet_amd.fit.fit_denoising``: batches, objective, clipping, Adam, the step log and the validation set all stay on the device, and
the host reads it once per ``print_freq`` steps.  The validation images are ``<test_path>/*.png`` (config key ``test_path``, default the
reference's ``test_data/CBSD68``); without any the test stage is skipped.  Two more optional config keys: ``steps_per_epoch`` (default
10000, the reference's dataset length over its batch size) and ``max_images`` (decode at most that many training images).

The whole pool lives in device memory (about 30 GB for the reference's four training sets).  JPEG decoding is PIL's: CBSD432 pixels may
differ from the reference's cv2 decode in the last bit where the two link different libjpeg builds.  ``--gpus N`` (or torchrun) trains
data-parallel as the reference's one process per device does: ``batch_size`` is the global batch, every rank builds its own pool, rank 0
prints, validates and saves.  ``--ema-decay X [--ema-warmup]`` (or the config keys ``ema_decay`` / ``ema_warmup``; the flags win) keeps an
exponential moving average of the weights on the device, validates on it and saves it as ``ema_state_dict``.

    python tools/train_denoising_syn.py --config configs/denoising_syn.json --save_dir train_record [--resume train_record/models/model_3.pth] [--gpus 8]
        [--ema-decay 0.999 [--ema-warmup]]
"""
import os
import sys
from pathlib import Path

import train_common as tc          # (the sibling module; importing it puts the repository root on sys.path)

TRAIN_SETS = (("CBSD_path", "*.jpg"), ("WED_path", "*.bmp"), ("Flickr", "*.png"), ("DIV2K", "*.png"))          # train_denoising_syn.py:113-116


def str2bool(v) -> bool:
    return v if isinstance(v, bool) else str(v).lower() in ("yes", "true", "t", "y", "1")


def build_net(args: dict, device):
    import torch
    from virnet_amd.networks import VIRAttResUNet
    torch.manual_seed(1234)          # train_denoising_syn.py:52-53: the seed before the network is initialised
    torch.cuda.manual_seed_all(1234)
    net = VIRAttResUNet(im_chn=args["im_chn"], sigma_chn=args["sigma_chn"], dep_S=args["dep_S"], n_feat=args["n_feat"],
                        n_resblocks=args["n_resblocks"], noise_avg=False, extra_mode=args["extra_mode"], noise_cond=str2bool(args["noise_cond"]))
    return net.to(device)


def main():
    args = tc.read_args("./configs/denoising_syn.json", "./train_record", "Path to save the model and log file", 15)
    from virnet_amd import datagen, fit
    device = tc.device("train_denoising_syn")
    net = build_net(args, device)
    tc.print_parameter_counts(net, ("SNet", "RNet"))
    files = []
    for key, pattern in TRAIN_SETS:
        if args.get(key):
            files += list(Path(args[key]).glob(pattern))
    files = sorted(str(x) for x in files)
    if args.get("max_images"):
        files = files[:int(args["max_images"])]
    print(f"Number of training image pairs: {len(files):d}", flush=True)
    if not files:
        sys.exit("no training images: point CBSD_path / WED_path / Flickr / DIV2K of the config at the image folders")
    pool = datagen.ImagePool(tc.read_images(files, int(args["patch_size"]), "train"), device)
    test_files = sorted(str(x) for x in Path(args.get("test_path", os.path.join("test_data", "CBSD68"))).glob("*.png"))
    val = None
    if test_files:
        val = datagen.SimulateTestSet(datagen.ImagePool(tc.read_images(test_files, 11, "test"), device))
    else:
        print("no validation images found: the test stage is skipped", flush=True)
    print(f"T_max = {args['epochs'] - args['warmup_epochs']:d}, eta_min={args.get('lr_min', 1e-6):.2e}")
    fit.fit_denoising(net, pool, args, val=val, save_dir=args["save_dir"], resume=tc.resume_path(args), log=lambda s: print(s, flush=True),
                      writer=tc.summary_writer(args))


if __name__ == "__main__":
    main()
