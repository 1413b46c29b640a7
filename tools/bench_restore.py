#!/usr/bin/env python
"""Times of tiled whole-image restoration (virnet_amd.restore) on one GPU, written up in profiles/restore_device.md.

For a seeded uint8 photograph (default 3000 x 4000 x 3, tile 512, overlap 32) it measures, after warm-up, in blocks that alternate between
the routes (median [min, max] over the blocks; device events, and a host clock around a block that ends in a synchronise):

  kernels   virnet_tile_gather over all tiles (one launch per 64) and virnet_tile_blend (uint8 HWC out), each in blocks of back-to-back
            launches, with the bytes each has to move (counted from the plan) over that time as a share of the 6.29 TB/s copy rate;
  glue      the stitching around an identity "forward" in chunks of 8 tiles, by three routes on the same grid:
            device  restore.restore_tiles + restore.blend (uint8 in, uint8 out),
            tiled   utils.tiling.forward_tiled on the float image (the slicing glue alone: torch.cat of slices in, slice writes out),
            script  the same plus what a script does around it on the device: uint8 HWC -> float NCHW before, clamp / quantise / HWC after;
  image     the whole restore.restore_image call for the denoising-syn configuration (synthetic weights), uint8 in, uint8 out.

One JSON line per measurement on stdout (and appended to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virnet_amd import restore  # noqa: E402
from virnet_amd.networks import VIRAttResUNet  # noqa: E402
from virnet_amd.utils.synth import synth_state_dict  # noqa: E402
from virnet_amd.utils.tiling import forward_tiled  # noqa: E402

COPY_RATE = 6.29e12        # bytes/s of a float4 device copy on this chip (the roof these kernels are held against)
SYN = dict(im_chn=3, sigma_chn=1, n_feat=[96, 192, 288], dep_S=5, n_resblocks=3, noise_cond=True, extra_mode="Input", noise_avg=False)


def timed_blocks(routes, blocks, calls):
    """routes: {name: fn}.  Per block and route: `calls` calls between two device events, then a synchronise.  ms per call."""
    ev = {k: [] for k in routes}
    wall = {k: [] for k in routes}
    for _ in range(blocks):
        for name, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / calls)
            ev[name].append(a.elapsed_time(b) / calls)
    return ev, wall


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def blend_read_bytes(p, c):
    """Bytes of the stack a blend launch reads: one float per used (row slot, column slot) pair per channel, plus the tables."""
    rows = (p.row_idx >= 0).sum(axis=1).astype(np.int64).sum()
    cols = (p.col_idx >= 0).sum(axis=1).astype(np.int64).sum()
    return int(rows * cols) * c * 4 + p.table_blob().nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--image-calls", type=int, default=3)
    ap.add_argument("--skip-image", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_restore needs a ROCm device (no CPU fallback)")
    H, W, C = args.height, args.width, 3
    rng = np.random.default_rng(0)
    u8 = torch.from_numpy(rng.integers(0, 256, (H, W, C), dtype=np.uint8)).cuda()
    lines = []

    def emit(**kw):
        kw.update(height=H, width=W, tile=args.tile, overlap=args.overlap)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    lin = restore.plan(H, W, args.tile, args.overlap, blend="linear")
    crop = restore.plan(H, W, args.tile, args.overlap, blend="crop")
    for p in (lin, crop):
        p.tables(u8.device)
    stack = restore.gather(u8, lin, 0, lin.T)
    identity = lambda t: t                                                     # noqa: E731

    # ---- the two kernels ------------------------------------------------------------------------------------------------------------
    routes = {"gather": lambda: restore.gather(u8, lin, 0, lin.T),
              "blend_linear_u8": lambda: restore.blend(stack, lin),
              "blend_crop_u8": lambda: restore.blend(stack, crop),
              "blend_linear_f32": lambda: restore.blend(stack, lin, out="float32", layout="chw")}
    for fn in routes.values():
        fn()
    ev, wall = timed_blocks(routes, args.blocks, args.calls)
    tile_px = lin.T * lin.th * lin.tw * C
    moved = {"gather": tile_px + tile_px * 4,
             "blend_linear_u8": blend_read_bytes(lin, C) + H * W * C,
             "blend_crop_u8": blend_read_bytes(crop, C) + H * W * C,
             "blend_linear_f32": blend_read_bytes(lin, C) + H * W * C * 4}
    for name in routes:
        ms = stats(ev[name])
        rate = moved[name] / (ms["median"] * 1e-3)
        emit(kind="kernel", name=name, tiles=lin.T, event_ms=ms, wall_ms=stats(wall[name]), bytes=moved[name], bytes_per_s=rate,
             share_of_copy_rate=rate / COPY_RATE)

    # ---- the glue around an identity forward ------------------------------------------------------------------------------------------
    x = (u8.permute(2, 0, 1).float() / 255.0)[None].contiguous()

    def device_route():
        return restore.blend(restore.restore_tiles(identity, u8, lin, batch=8), lin)

    def device_crop_route():
        return restore.blend(restore.restore_tiles(identity, u8, crop, batch=8), crop)

    def tiled_route():
        return forward_tiled(identity, x, tile=args.tile, overlap=args.overlap, batch=8)

    def script_route():
        xx = (u8.permute(2, 0, 1).float() / 255.0)[None].contiguous()
        y = forward_tiled(identity, xx, tile=args.tile, overlap=args.overlap, batch=8)
        return (y[0].clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).permute(1, 2, 0).contiguous()

    routes = {"device": device_route, "device_crop": device_crop_route, "tiled": tiled_route, "script": script_route}
    a, b = device_crop_route(), script_route()
    same = bool(torch.equal(a, b))                                             # (identity forward: crop mode must give the image back)
    assert same and torch.equal(a, u8), "the routes disagree"
    for fn in routes.values():
        fn()
    ev, wall = timed_blocks(routes, args.blocks, max(1, args.calls // 2))
    for name in routes:
        emit(kind="glue", name=name, tiles=lin.T, batch=8, event_ms=stats(ev[name]), wall_ms=stats(wall[name]))

    # ---- the whole call ---------------------------------------------------------------------------------------------------------------
    if not args.skip_image:
        net = VIRAttResUNet(**SYN)
        net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
        net = net.cuda().eval()
        auto = restore.auto_tile(H, W, restore.widest_channels(net), 1, multiple=4)
        call = lambda: restore.restore_image(net, u8, tile=args.tile, overlap=args.overlap)      # noqa: E731
        out = call()
        assert out.dtype == torch.uint8 and out.shape == (H, W, C)
        ev, wall = timed_blocks({"restore_image": call}, args.image_calls, 1)
        emit(kind="image", name="restore_image", config="denoising-syn", tiles=lin.T, batch=8, auto_tile=auto, event_ms=stats(ev["restore_image"]),
             wall_ms=stats(wall["restore_image"]), megapixels_per_s=H * W / 1e6 / (statistics.median(wall["restore_image"]) * 1e-3),
             resident_bytes=lin.resident_bytes(1, (3,), 1, 8))
    if args.out:
        with open(args.out, "a") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
