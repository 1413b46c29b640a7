"""The cases of tests/golden/jpeg.npz (written by tests/golden/make_jpeg_golden.py from Pillow's libjpeg-turbo), shared by
tests/test_jpeg_host.py and tests/test_jpeg_gpu.py: loaded once, never modified."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=1)
def fixture():
    with np.load(os.path.join(GOLDEN, "jpeg.npz")) as f:
        data = {k: f[k] for k in f.files}
    for v in data.values():
        v.setflags(write=False)
    return data


def sizes():
    return [tuple(int(v) for v in s) for s in fixture()["sizes"]]


def cases(h, w):
    """[(kind, quality, input uint8 [h,w,3], Pillow's decoded output uint8 [h,w,3])] of one size: every kind at every quality."""
    f = fixture()
    out = []
    for kind in f["kinds"]:
        im = f[f"in_{h}x{w}_{kind}"]
        for i, q in enumerate(f["qualities"]):
            stored = f[f"out_{h}x{w}_{kind}"][i].transpose(1, 2, 0)
            out.append((str(kind), int(q), im, stored + im if q >= f["diff_from"] else stored))      # uint8: (out - in) + in mod 256
    return out
