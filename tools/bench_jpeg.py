#!/usr/bin/env python
"""Time of the device JPEG round trip (virnet_amd/jpeg.py) from device events, next to the host route it replaces, in one process.

For a batch of N = 32 images at the LR sizes 48 (the x4 training patch), 64, 128 and 256:

  * ``jpeg.jpeg_compress`` on float32 and on uint8 CUDA batches, the qualities given as an int32 tensor (median of ``--repeats`` blocks of
    ``--calls`` calls, after warm-up), with the bytes the two launches move at least (source, the uint8 workspace written and read once,
    destination) and the rate that makes;
  * the host path, each part on its own: ``jpeg.roundtrip_np`` per image, Pillow's encode + decode of the same images on one thread when
    Pillow is importable, and the device -> host -> device copies that surround a host round trip of the float32 batch.

Prints one JSON line per size.

    python tools/bench_jpeg.py [--repeats 15] [--calls 20] [--batch 32] [--sizes 48 64 128 256] [--qf 40]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virnet_amd import eval as veval  # noqa: E402
from virnet_amd import jpeg  # noqa: E402


def _block_ms(step, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def _device_ms(step, repeats, calls, warmup=5):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = [_block_ms(step, calls) for _ in range(repeats)]
    return statistics.median(ms), min(ms), max(ms)


def _host_ms(step, repeats):
    step()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        step()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def _pillow_roundtrip():
    try:
        from PIL import Image
    except ImportError:
        return None

    def roundtrip(im, q):
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, format="JPEG", quality=q)
        with Image.open(io.BytesIO(buf.getvalue())) as dec:
            return np.asarray(dec.convert("RGB"))
    return roundtrip


def images(n, size, seed):
    """smooth colour gradients plus noise: float32 [n,3,size,size] in [0,1]"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size] / size
    base = np.stack([0.5 + 0.4 * np.sin(6.0 * xx + 3.0 * yy), yy, 1.0 - xx])
    return np.clip(base[None] + g.normal(0.0, 0.06, (n, 3, size, size)), 0.0, 1.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[48, 64, 128, 256])
    ap.add_argument("--qf", type=int, default=40)
    ap.add_argument("--host-images", type=int, default=4, help="images per timed host block (the host paths are per image)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_jpeg needs a ROCm device"
    torch.set_num_threads(1)
    pillow = _pillow_roundtrip()
    n = args.batch
    for size in args.sizes:
        host = images(n, size, size)
        x32 = torch.from_numpy(host).cuda()
        x8 = torch.from_numpy(veval.img_as_ubyte(host)).cuda()
        qt = torch.full((n,), args.qf, dtype=torch.int32).cuda()
        jpeg.warm(x32.device)
        row = {"row": "jpeg_roundtrip", "shape": [n, 3, size, size], "qf": args.qf, "calls_per_block": args.calls, "blocks": args.repeats}
        # the device result is the host definition's (first image), and Pillow's when it is there
        hwc8 = np.ascontiguousarray(veval.img_as_ubyte(host[0]).transpose(1, 2, 0))
        dev8 = jpeg.jpeg_compress(x8, qt)[0].permute(1, 2, 0).cpu().numpy()
        row["differing_bytes_vs_roundtrip_np"] = int((dev8 != jpeg.roundtrip_np(hwc8, args.qf)).sum())
        if pillow is not None:
            row["differing_bytes_vs_pillow"] = int((dev8 != pillow(hwc8, args.qf)).sum())
        ws = n * (size * size + 2 * ((size + 1) // 2) ** 2)
        for name, x, elt in (("float32", x32, 4), ("uint8", x8, 1)):
            med, lo, hi = _device_ms(lambda: jpeg.jpeg_compress(x, qt), args.repeats, args.calls)
            moved = 2 * n * 3 * size * size * elt + 2 * ws
            row[f"device_ms_{name}"] = round(med, 4)
            row[f"device_ms_{name}_range"] = [round(lo, 4), round(hi, 4)]
            row[f"device_us_per_image_{name}"] = round(med * 1e3 / n, 3)
            row[f"device_min_bytes_{name}"] = moved
            row[f"device_gb_per_s_{name}"] = round(moved / (med * 1e-3) / 1e9, 1)
        k = min(args.host_images, n)
        ims = [np.ascontiguousarray(veval.img_as_ubyte(host[i]).transpose(1, 2, 0)) for i in range(k)]
        reps = max(3, args.repeats // 3)
        row["host_ms_per_image_roundtrip_np"] = round(_host_ms(lambda: [jpeg.roundtrip_np(im, args.qf) for im in ims], reps) / k, 3)
        if pillow is not None:
            row["host_ms_per_image_pillow"] = round(_host_ms(lambda: [pillow(im, args.qf) for im in ims], reps) / k, 3)

        def copies():
            back = x32.cpu()
            torch.cuda.synchronize()
            return back.cuda()
        t = []
        for _ in range(args.repeats + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            copies()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        row["copies_ms_batch_float32"] = round(statistics.median(t[2:]), 4)
        if pillow is not None:
            row["host_route_ms_batch_pillow"] = round(row["host_ms_per_image_pillow"] * n + row["copies_ms_batch_float32"], 3)
            row["speedup_vs_host_route_float32"] = round(row["host_route_ms_batch_pillow"] / row["device_ms_float32"], 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
