#!/usr/bin/env python
"""Golden values for virnet_amd/jpeg.py, produced by Pillow's libjpeg-turbo: ``Image.save(format="JPEG", quality=q)`` with everything else
at its default (4:2:0, slow-integer DCT, baseline tables), then ``Image.open`` (fancy upsampling).  Run on the CPU:

    python tests/golden/make_jpeg_golden.py

Writes tests/golden/jpeg.npz:
  * ``in_<h>x<w>_<kind>``           uint8 [h,w,3] inputs: uniform noise, smooth + noise, saturated 0/255 noise, a one-pixel checkerboard
  * ``out_<h>x<w>_<kind>``          uint8 [qualities,3,h,w]: Pillow's decoded outputs as planes; for the qualities from DIFF_FROM up they are
                                    stored as (out - in) mod 256, which deflates better there (tests/jpeg_cases.py undoes it)
  * ``tables``                      uint8 [101,2,64]: Pillow's (luma, chroma) quantisation tables of qualities 1..100, natural order
  * ``sizes``, ``kinds``, ``qualities``, ``diff_from``, ``versions`` (Pillow and libjpeg-turbo)
The sizes are the smallest that reach every padding case: 1x1 and 7x9 are partial in both planes, 8x8 has one luma block and a padded chroma
block, 17x33 / 37x51 are odd (ceil chroma, replicated right / bottom MCU), 31x16 mixes even and odd, 40x56 has several MCUs with the chroma
halo crossing their borders in both axes; 2x3 and 9x4 have chroma planes at most two samples wide, which the library upsamples by
repetition instead of the triangle filter.  The file is about 300 KB: the decoded noise images are as incompressible as their inputs.

When cv2 and the reference (its checkout named by VIRNET_REFERENCE) can be imported, every case is also pushed through the reference's own
``util_image.jpeg_compress`` and must give the same bytes; without cv2 that equality rests on both libraries bundling libjpeg-turbo with
its defaults.
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (31, 16), (37, 51), (40, 56), (2, 3), (9, 4)]
KINDS = ["uniform", "smooth", "saturated", "checker"]
QUALITIES = [1, 10, 40, 75, 95, 100]
DIFF_FROM = 25          # qualities from here up are stored as the difference to the input
# zigzag position -> natural index (JPEG specification, figure A.6): Pillow reports its tables in the file's zigzag order
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def encode(im: np.ndarray, q: int) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(im).save(buf, format="JPEG", quality=q)
    return buf.getvalue()


def pillow_roundtrip(im: np.ndarray, q: int) -> np.ndarray:
    with Image.open(io.BytesIO(encode(im, q))) as dec:
        return np.asarray(dec.convert("RGB"), dtype=np.uint8)


def pillow_tables(q: int) -> np.ndarray:
    with Image.open(io.BytesIO(encode(np.zeros((8, 8, 3), dtype=np.uint8), q))) as dec:
        qt = dec.quantization
    out = np.zeros((2, 64), dtype=np.uint8)
    for comp in (0, 1):
        raw = np.asarray(list(qt[comp]), dtype=np.uint8)
        # newer Pillow versions already hand the tables out in natural order; older ones in zigzag order
        natural = raw if _TABLES_NATURAL else raw[np.argsort(ZIGZAG)]
        out[comp] = natural
    return out


def _tables_are_natural() -> bool:
    """Quality 50 is the Annex K table itself: its second entry is 11 in natural order, and in zigzag order too (16, 11, 12 vs 16, 11, 10):
    the third entry tells them apart."""
    with Image.open(io.BytesIO(encode(np.zeros((8, 8, 3), dtype=np.uint8), 50))) as dec:
        third = list(dec.quantization[0])[2]
    assert third in (10, 12), third
    return third == 10


_TABLES_NATURAL = _tables_are_natural()


def make_input(kind: str, h: int, w: int, g: np.random.Generator) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "uniform":
        return g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "smooth":
        base = np.stack([40 + 3 * yy + 2 * xx, 220 - 4 * xx + yy, 128 + 60 * np.sin(0.3 * xx + 0.2 * yy)], axis=-1)
        return np.clip(np.rint(base + g.normal(0.0, 4.0, (h, w, 3))), 0, 255).astype(np.uint8)
    if kind == "saturated":
        return (g.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if kind == "checker":
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    raise ValueError(kind)


def reference_jpeg_compress():
    """The reference's util_image.jpeg_compress when cv2 and the reference are importable, else None."""
    try:
        import cv2  # noqa: F401
    except ImportError:
        return None
    ref = os.environ.get("VIRNET_REFERENCE", "")
    if not os.path.isdir(ref):
        return None
    sys.path.insert(0, ref)
    try:
        from utils import util_image
    except ImportError:
        return None
    return lambda im, q: util_image.jpeg_compress(im, int(q), chn_in="rgb")


def main():
    g = np.random.default_rng(20240611)
    ref = reference_jpeg_compress()
    out = {"sizes": np.asarray(SIZES, dtype=np.int32), "kinds": np.asarray(KINDS), "qualities": np.asarray(QUALITIES, dtype=np.int32),
           "versions": np.asarray(["Pillow " + PIL.__version__, "libjpeg-turbo " + str(features.version("libjpeg_turbo"))]),
           "diff_from": np.asarray(DIFF_FROM, dtype=np.int32),
           "tables": np.stack([np.zeros((2, 64), dtype=np.uint8)] + [pillow_tables(q) for q in range(1, 101)])}
    assert features.check_feature("libjpeg_turbo"), "this fixture pins libjpeg-turbo's output"
    for h, w in SIZES:
        for kind in KINDS:
            im = make_input(kind, h, w, g)
            out[f"in_{h}x{w}_{kind}"] = im
            decoded = []
            for q in QUALITIES:
                dec = pillow_roundtrip(im, q)
                assert dec.shape == im.shape
                if ref is not None:
                    assert np.array_equal(ref(im, q), dec), f"cv2 and Pillow differ on {h}x{w} {kind} q={q}"
                decoded.append((dec - im if q >= DIFF_FROM else dec).transpose(2, 0, 1))      # uint8 arithmetic: (out - in) mod 256
            out[f"out_{h}x{w}_{kind}"] = np.stack(decoded)
    path = os.path.join(HERE, "jpeg.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays, {out['versions'].tolist()}, "
          f"{'checked against the reference through cv2' if ref is not None else 'cv2 not importable: Pillow only'}")


if __name__ == "__main__":
    main()
