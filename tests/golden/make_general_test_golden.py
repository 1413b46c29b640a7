#!/usr/bin/env python
"""Golden validation samples for virnet_amd/datagen.py (GeneralTestSet, general_test_np, general_noise), produced by the REFERENCE's own
``GeneralTest`` (datasets/SISRDatasets.py:124-207) on two small crops of the tests/golden/cbsd68 PNGs written as BMP to a temporary folder:
one 44 x 60 and one 60 x 44, so that h_max = w_max = 60 and the noise array ([30,30,3] at sf 2, [15,15,3] at sf 4) is read with a row
stride wider than either LR image and with fewer rows than it holds.  Cases: sf 2 / direct and sf 4 / bicubic, Gaussian noise, and
``sf2s``: sf 2 / bicubic with ``kernel_shift=True`` -- the half-pixel centre makes the kernel asymmetric, so the direction in which it is
applied (a true convolution) shows.

Build container only: imports the reference (its checkout named by VIRNET_REFERENCE) at generation time; no test reads it.  The stubs are
those of make_simulate_test_golden.py (``cv2.imread`` served by PIL in BGR order, ``cv2.cvtColor`` by a channel flip; nothing on this
path resizes).  scipy and the reference's vendored ResizeRight are the real ones.

The JPEG variant has NO reference golden: it would need ``cv2.imencode`` / ``cv2.imdecode`` served by Pillow, which makes the round trip
circular (make_jpeg_golden.py pins Pillow's libjpeg-turbo bytes directly and compares with cv2 only where cv2 is installed).  It is held to
``sisr_eval.synthesize_tail_np(qf=40)`` on the Gaussian case's inputs instead, whose codec tests/golden/jpeg.npz pins.

Writes tests/golden/general_test.npz: ``files``, ``seed``, ``u8_<i>`` (the crops, uint8 HWC), and per case ``<case>_sf``,
``<case>_downsampler``, ``<case>_shift``, ``<case>_noise`` (the set's fp32 noise array), ``<case>_hr_<i>``, ``<case>_lr_<i>`` (fp32 CHW) and
``<case>_kinfo_<i>`` (fp32 [3]): what ``GeneralTest.__getitem__`` returned.
"""
import glob
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VIRNET_REFERENCE")
if not REF or not os.path.isdir(REF):
    sys.exit("set VIRNET_REFERENCE to a checkout of the reference")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, REF)
from virnet_amd import eval as veval  # noqa: E402

for name in ("cv2", "thop", "lpips", "lmdb", "h5py", "skimage", "skimage.metrics", "skimage.color"):
    sys.modules.setdefault(name, types.ModuleType(name))
sk = sys.modules["skimage"]
sk.img_as_float32 = veval.img_as_float32
sk.img_as_ubyte = veval.img_as_ubyte
sk.img_as_float64 = None
sys.modules["skimage.metrics"].structural_similarity = None
sys.modules["thop"].profile = None
cv2 = sys.modules["cv2"]
cv2.IMREAD_COLOR, cv2.IMREAD_UNCHANGED, cv2.IMREAD_GRAYSCALE, cv2.COLOR_BGR2RGB, cv2.COLOR_RGB2BGR = 1, -1, 0, 4, 4


def _imread(path, flag=1):
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[:, :, ::-1])


cv2.imread = _imread
cv2.cvtColor = lambda im, code: np.ascontiguousarray(im[:, :, ::-1])

from datasets.SISRDatasets import GeneralTest  # noqa: E402  (the reference)

SEED, K = 10000, 21
sources = sorted(glob.glob(os.path.join(HERE, "cbsd68", "*.png")))[:2]
crops = ((44, 60, 17, 101), (60, 44, 203, 33))          # (h, w, top, left)
out = {"seed": np.asarray(SEED, dtype=np.int64)}
with tempfile.TemporaryDirectory() as tmp:
    for i, (src, (h, w, top, left)) in enumerate(zip(sources, crops)):
        u8 = veval.imread_rgb_uint8(src)[top:top + h, left:left + w]
        assert u8.shape == (h, w, 3)
        Image.fromarray(u8).save(os.path.join(tmp, f"crop_{i}.bmp"))
        out[f"u8_{i}"] = np.ascontiguousarray(u8)
    for case, sf, down, shift in (("sf2", 2, "direct", False), ("sf4", 4, "bicubic", False), ("sf2s", 2, "bicubic", True)):
        ds = GeneralTest(tmp, sf=sf, k_size=K, kernel_shift=shift, downsampler=down, seed=SEED, noise_type="Gaussian")
        assert len(ds) == 2 and ds.fixed_noise.shape == (60 // sf, 60 // sf, 3) and ds.fixed_noise.dtype == np.float32
        out["files"] = np.asarray([os.path.basename(f) for f in ds.hr_path_list])
        out[f"{case}_sf"], out[f"{case}_downsampler"], out[f"{case}_noise"] = np.asarray(sf, dtype=np.int64), np.asarray(down), ds.fixed_noise
        out[f"{case}_shift"] = np.asarray(shift)
        for i in range(len(ds)):
            hr, lr, kinfo = ds[i]
            out[f"{case}_hr_{i}"], out[f"{case}_lr_{i}"], out[f"{case}_kinfo_{i}"] = hr.numpy(), lr.numpy(), kinfo.numpy()
            print(case, i, hr.shape, hr.dtype, lr.shape, lr.dtype, kinfo.tolist(), float(lr.mean()))

path = os.path.join(HERE, "general_test.npz")
np.savez_compressed(path, **out)
print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")
