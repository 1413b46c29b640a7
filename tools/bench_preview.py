#!/usr/bin/env python
"""Cost of the training previews (virnet_amd/preview.py, csrc/preview.hip).

``--part event`` times ONE preview event, from device tensors to uint8 arrays on the host, two ways:

  * ``device``: the grids of the event through ``preview.grids`` (two launches each, one buffer) and ONE ``preview.to_host``;
  * ``torch``: the same event written in torch ops, as a user of the package had to before -- per grid a clone, the clamp, per-image
    ``amin`` / ``amax``, subtract, divide, the repeat of a single plane, the paste into a zero canvas, ``mul(255).clamp(0, 255).to(uint8)``,
    the permute to HWC and ``.cpu()`` -- torchvision's ``make_grid(normalize=True, scale_each=True)`` plus the writer's conversion, restated
    here (torchvision is not needed).  It uses nothing of the preview unit, so it runs the same on a library without it.

  denoise: 5 grids -- four of 32 x 3 x 128 x 128 and one of 32 x 1 x 128 x 128;  sisr: 6 grids -- two of 16 x 3 x 192 x 192, one of
  16 x 3 x 48 x 48, three of 16 x 1 x 21 x 21 (for ``device`` two of them come from ``preview.kernel_from_kinfo``, for ``torch`` they are
  given: the comparator is not charged for the kernel formula).

The two routes alternate call by call inside a pass, ``--reps`` calls each after warm-up, every call timed on the host clock between two
device synchronisations (the host copy is the subject); two passes; per route the median of each pass and (max - min) / median over the
pass.  One JSON line per event kind.

``--part loop`` times the denoising training loop of tools/bench_trainloop.py's ``fit`` route (batch 16, 128 x 128, the log read every 100
steps) without a writer and with one that receives a preview event every ``--preview-every`` steps (the loop's own interval at
``print_freq=100`` is 5000 steps; a smaller one bounds the cost from above in less time), alternating blocks of ``--calls`` steps.

    python tools/bench_preview.py [--part event|loop|both] [--reps 30] [--calls 100] [--repeats 5] [--preview-every 100]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

EVENTS = {"denoise": [((32, 3, 128, 128), (0.0, 1.0)), ((32, 3, 128, 128), None), ((32, 1, 128, 128), None), ((32, 1, 128, 128), None),
                      ((32, 3, 128, 128), None)],
          "sisr": [((16, 3, 192, 192), None), ((16, 3, 192, 192), None), ((16, 1, 21, 21), None), ((16, 3, 48, 48), None), ((16, 1, 21, 21), None),
                   ((16, 1, 21, 21), None)]}


def torch_grid(torch, x, clamp, nrow=8, padding=2):
    """make_grid(normalize=True, scale_each=True) and the writer's uint8 HWC conversion in torch ops, then ``.cpu()``"""
    x = x.clone()
    if clamp is not None:
        x.clamp_(*clamp)
    lo, hi = x.amin(dim=(1, 2, 3), keepdim=True), x.amax(dim=(1, 2, 3), keepdim=True)
    x = x.sub_(lo).div_((hi - lo).clamp_(min=1e-5))
    if x.shape[1] == 1:
        x = x.expand(-1, 3, -1, -1)
    b, _, h, w = x.shape
    xmaps = min(nrow, b)
    ymaps = -(-b // xmaps)
    canvas = torch.zeros((3, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding), dtype=x.dtype, device=x.device)
    for k in range(b):
        y0, x0 = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        canvas[:, y0:y0 + h, x0:x0 + w] = x[k]
    return canvas.mul(255).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()


def event(kind, reps, passes=2):
    import torch
    from virnet_amd import preview as pv
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(shape, generator=g).cuda() * 0.3 + 0.5 for shape, _ in EVENTS[kind]]
    clamps = [c for _, c in EVENTS[kind]]
    kinfo = torch.tensor([[2.0, 5.0, 0.3]] * 16).cuda()

    def device():
        specs = [dict(x=x, clamp=c) for x, c in zip(xs, clamps)]
        if kind == "sisr":
            specs[2]["x"], specs[5]["x"] = pv.kernel_from_kinfo(kinfo, 21, 4, False), pv.kernel_from_kinfo(kinfo, 21, 4, True)
        return pv.to_host(pv.grids(specs))

    def plain():
        return [torch_grid(torch, x, c) for x, c in zip(xs, clamps)]

    routes = {"device": device, "torch": plain}
    for call in routes.values():
        for _ in range(3):
            call()
    row = {"row": "preview_event", "event": kind, "grids": len(xs), "host_bytes": int(sum(a.size for a in device())), "reps": reps, "passes": passes}
    for p in range(passes):
        ms = {name: [] for name in routes}
        for _ in range(reps):
            for name, call in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                ms[name].append(1e3 * (time.perf_counter() - t0))
        for name, v in ms.items():
            row[f"{name}_ms_pass{p}"] = round(statistics.median(v), 3)
            row[f"{name}_spread_pass{p}"] = round((max(v) - min(v)) / statistics.median(v), 3)
    row["torch_over_device"] = round(statistics.mean(row[f"torch_ms_pass{p}"] for p in range(passes)) /
                                     statistics.mean(row[f"device_ms_pass{p}"] for p in range(passes)), 2)
    print(json.dumps(row), flush=True)


class _Sink:
    def add_scalar(self, tag, value, step):
        pass

    def add_image(self, tag, image, step, dataformats="HWC"):
        self.last = image.shape


def loop(batch, calls, repeats, preview_every, read_every=100):
    import random
    import torch
    import bench
    import bench_trainloop as bt
    from virnet_amd import fit
    from virnet_amd.trainlog import StepLog
    dev = torch.device("cuda", torch.cuda.current_device())
    c = fit.read_config(dict(bt.CFG, batch_size=batch))
    pool = bt._pool(dev)
    alpha0 = (0.5 * torch.tensor([c["var_window"] ** 2], dtype=torch.float32)).to(dev)
    runs = {}
    for route in ("fit", "fit_previews"):
        net, sd = bench.build_net(dev, "denoise")
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).train()
        opt = fit._optimizer(net, c, ("rnet", "snet"))
        log, rng, state, sink = StepLog(fit.LOG_NAMES, read_every, c["steps_per_epoch"], dev), random.Random(0), {"ii": 0}, _Sink()
        step_img = {"train": 0}

        def run(n, net=net, opt=opt, log=log, rng=rng, state=state, sink=sink, step_img=step_img, previews=route == "fit_previews"):
            for _ in range(n):
                ii = state["ii"]
                keep = {} if previews and (ii + 1) % preview_every == 0 else None
                fit.train_step(net, opt, pool, c, rng, 0, ii, alpha0, False, log, keep=keep)
                if (ii + 1) % read_every == 0:
                    state["rows"] = log.read()
                if keep is not None:
                    fit._emit(sink, fit._denoise_train_preview(keep), step_img, "train")
                state["ii"] = ii + 1
        runs[route] = run
    rate = bt._ab(runs, batch, repeats, calls, warmup=10)
    row = {"row": "preview_loop", "shape": [batch, 3, c["patch_size"], c["patch_size"]], "calls_per_block": calls, "blocks": repeats,
           "log_read_every": read_every, "preview_every": preview_every}
    for name, v in rate.items():
        row[f"images_per_s_{name}"] = round(statistics.median(v), 1)
        row[f"images_per_s_{name}_range"] = [round(min(v), 1), round(max(v), 1)]
    a = rate["fit"]
    row["spread_fit"] = round((max(a) - min(a)) / statistics.median(a), 4)
    row["previews_over_fit"] = round(statistics.median(rate["fit_previews"]) / statistics.median(a), 4)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["event", "loop", "both"])
    ap.add_argument("--reps", type=int, default=30, help="timed calls per route and pass of the event part")
    ap.add_argument("--calls", type=int, default=100, help="steps per timed block of the loop part")
    ap.add_argument("--repeats", type=int, default=5, help="blocks per route of the loop part")
    ap.add_argument("--preview-every", type=int, default=100, help="steps between two preview events of the loop part (the loop's own: 5000)")
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    os.environ["VIRNET_CONV_FORM"] = "bf16"          # (the training step's operand form, as bench_trainloop.py's default; read at first plan)
    import torch
    assert torch.cuda.is_available(), "bench_preview needs a ROCm device"
    if args.part in ("event", "both"):
        for kind in EVENTS:
            event(kind, args.reps)
    if args.part in ("loop", "both"):
        loop(args.batch, args.calls, args.repeats, args.preview_every)


if __name__ == "__main__":
    main()
