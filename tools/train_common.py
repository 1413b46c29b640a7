"""What the three training drivers (train_denoising_syn.py, train_denoising_real.py, train_sisr.py) share: the flags, the config print,
the ranks of a data-parallel run (``--gpus N`` or torchrun), the device, the parameter counts, the image decoder, the resume check and the
summary writer of ``--previews``."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


MAX_RANKS = 16          # processes of one job that may hold the device open together


def parse_flags(argv, config: str, save_dir: str, save_help: str, config_first: bool = False):
    """--save_dir / --config / --resume (defaults and help text as given) and --gpus N."""
    ap = argparse.ArgumentParser()
    flags = [(("--save_dir",), dict(default=save_dir, type=str, metavar="PATH", help=save_help)),
             (("--config",), dict(type=str, default=config, help="Path for the config file"))]
    for names, kw in reversed(flags) if config_first else flags:
        ap.add_argument(*names, **kw)
    ap.add_argument("--resume", type=str, default=None, help="checkpoint to continue from (default: the config's 'resume')")
    ap.add_argument("--gpus", type=int, default=None, metavar="N",
                    help=f"train data-parallel on N devices (1..{MAX_RANKS}): the driver starts N fresh processes of itself, one per device; "
                         "the config's batch_size is the global batch.  Under torchrun (RANK / WORLD_SIZE set) leave it out")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="X",
                    help="keep an exponential moving average of the weights with decay X (0 <= X < 1; 0: off), validate on it and save it as "
                         "'ema_state_dict' (default: the config's 'ema_decay', off when absent)")
    ap.add_argument("--ema-warmup", action="store_true", default=None,
                    help="let the decay grow as min(X, (1 + t) / (10 + t)) over the first updates (default: the config's 'ema_warmup')")
    ap.add_argument("--previews", type=str, default=None, metavar="DIR",
                    help="write the reference's summaries -- the loss and test scalars as DIR/scalars.jsonl, the image grids of its "
                         "tensorboard previews as DIR/images/<tag>/<step>.png -- formed on the device (virnet_amd/preview.py; default: none)")
    opts = ap.parse_args(argv)
    if opts.gpus is not None and not 1 <= opts.gpus <= MAX_RANKS:
        ap.error(f"--gpus {opts.gpus}: 1..{MAX_RANKS} ranks are supported")
    if opts.ema_decay is not None and not 0.0 <= opts.ema_decay < 1.0:
        ap.error(f"--ema-decay {opts.ema_decay}: 0 <= X < 1 is expected")
    return opts


def apply_ema_flags(args: dict, opts) -> dict:
    """``--ema-decay`` / ``--ema-warmup`` override the config's ``ema_decay`` / ``ema_warmup`` (virnet_amd/fit.py reads both)."""
    if opts.ema_decay is not None:
        args["ema_decay"] = opts.ema_decay
    if opts.ema_warmup:
        args["ema_warmup"] = True
    return args


def rank_commands(n: int, script: str, argv, port: int, environ=None):
    """The N child processes of ``--gpus N``: [(command, environment)] -- this driver again without the flag, under the torchrun
    variables of rank r.  The children are fresh interpreters: the parent has not opened the device and keeps running as their monitor."""
    if not 1 <= n <= MAX_RANKS:
        raise ValueError(f"{n} ranks: 1..{MAX_RANKS} are supported")
    rest, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a == "--gpus":
            skip = True
        elif not a.startswith("--gpus="):
            rest.append(a)
    base = dict(os.environ if environ is None else environ)
    out = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        out.append(([sys.executable, script] + rest, env))
    return out


def launch_ranks(n: int) -> int:
    """Run this driver as N ranks and wait for them -> the job's exit code.  A rank that fails ends its peers."""
    import socket
    import subprocess
    import time
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [subprocess.Popen(cmd, env=env) for cmd, env in rank_commands(n, os.path.abspath(sys.argv[0]), sys.argv[1:], port)]
    try:
        while True:
            codes = [p.poll() for p in procs]
            bad = [c for c in codes if c not in (None, 0)]
            if bad or all(c == 0 for c in codes):
                return bad[0] if bad else 0
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()


def read_args(config: str, save_dir: str, save_help: str, width: int, config_first: bool = False) -> dict:
    """Parse the flags, read the config file, let the flags override its ``save_dir`` and ``resume``, and print every key in a column of
    ``width``.  -> the config dict.  ``--gpus N`` (N > 1, outside torchrun) never returns: the process becomes the monitor of N ranks.
    Inside a rank (RANK / WORLD_SIZE set, by torchrun or by that monitor) the process group is joined and ranks above 0 print nothing."""
    opts = parse_flags(sys.argv[1:], config, save_dir, save_help, config_first)
    if opts.gpus is not None and opts.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(opts.gpus))
    from virnet_amd import dist as vdist, fit
    timeout = os.environ.get("VIRNET_DIST_TIMEOUT")
    rank, _, world = vdist.init(timeout=float(timeout) if timeout else None)
    if world > 1 and rank > 0:
        sys.stdout = open(os.devnull, "w")
    args = fit.load_config(opts.config)
    args["save_dir"] = opts.save_dir
    if opts.resume is not None:
        args["resume"] = opts.resume
    apply_ema_flags(args, opts)
    if opts.previews is not None:
        args["previews"] = opts.previews
    for key, value in args.items():
        print(f"{key:<{width}s}: {value}")
    return args


def summary_writer(args: dict):
    """``--previews DIR``: a ``preview.FolderWriter`` on DIR for the loop's ``writer=`` (rank 0 of a data-parallel job; None otherwise)."""
    if not args.get("previews") or int(os.environ.get("RANK", "0")) != 0:
        return None
    from virnet_amd.preview import FolderWriter
    return FolderWriter(args["previews"])


def device(who: str):
    import torch
    assert torch.cuda.is_available(), f"{who} needs a ROCm device"
    return torch.device("cuda", torch.cuda.current_device())


def print_parameter_counts(net, names) -> None:
    for name in names:
        print(f"Number of parameters in {name}: {sum(p.numel() for p in getattr(net, name).parameters()) / 1000 ** 2:.2f}M", flush=True)


def read_images(paths, smallest: int, what: str):
    from virnet_amd import eval as veval
    images = []
    for p in paths:
        im = veval.imread_rgb_uint8(str(p))          # (grey files come back as three equal channels, as GeneralTest stacks them)
        if min(im.shape[:2]) < smallest:
            print(f"{what}: skipping {p} ({im.shape[0]}x{im.shape[1]}, smaller than {smallest})", flush=True)
            continue
        images.append(im)
    return images


def resume_path(args: dict):
    """The config's ``resume`` (None when empty); a path that is no file ends the run with the reference's message."""
    resume = args.get("resume") or None
    if resume and not os.path.isfile(resume):
        sys.exit("Please provide corrected model path!")
    return resume
