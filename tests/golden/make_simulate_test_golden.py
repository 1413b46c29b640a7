#!/usr/bin/env python
"""Golden validation samples for virnet_amd/datagen.py (SimulateTestSet, simulate_test_np), produced by the REFERENCE's own
``SimulateTest`` (datasets/DenoisingDatasets.py:255-296) on two small crops of the tests/golden/cbsd68 PNGs written to a temporary folder:
one 40 x 56 and one 56 x 40, so that h_max = w_max = 56 and the noise array is read with a row stride wider than either image and with
fewer rows than it holds.

Build container only: imports the reference (its checkout named by VIRNET_REFERENCE) at generation time; no test reads it.  The stubs are
those of make_datagen_golden.py (``cv2.imread`` served by PIL in BGR order, ``cv2.cvtColor`` by a channel flip), plus
  * ``cv2.resize(..., INTER_NEAREST_EXACT)`` served by ``virnet_amd.eval.resize_nearest_exact``.  That one step is therefore CIRCULAR: the
    golden pins the noise array, the sigma map, the float conversion, the order of the roundings and the strides, not the nearest-exact
    index rule, which tests/test_fit_host.py holds to its written definition instead.

Writes tests/golden/simulate_test.npz: ``files``, ``seed``, ``u8_<i>`` (the crops, uint8 HWC), ``noise`` ([56,56,3] fp32), ``sigma_map``
([256,256] fp32), ``noisy_<i>``, ``gt_<i>`` (fp32 CHW, what ``SimulateTest.__getitem__`` returned).
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
cv2.INTER_NEAREST_EXACT = 6


def _imread(path, flag=1):
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[:, :, ::-1])


def _resize(a, dsize, interpolation=None):
    assert interpolation == cv2.INTER_NEAREST_EXACT
    return veval.resize_nearest_exact(a, dsize[1], dsize[0])          # (circular: see the module docstring)


cv2.imread = _imread
cv2.cvtColor = lambda im, code: np.ascontiguousarray(im[:, :, ::-1])
cv2.resize = _resize

from datasets.DenoisingDatasets import SimulateTest  # noqa: E402  (the reference)

SEED = 1000
sources = sorted(glob.glob(os.path.join(HERE, "cbsd68", "*.png")))[:2]
crops = ((40, 56, 17, 101), (56, 40, 203, 33))          # (h, w, top, left)
out = {"seed": np.asarray(SEED, dtype=np.int64)}
with tempfile.TemporaryDirectory() as tmp:
    files = []
    for i, (src, (h, w, top, left)) in enumerate(zip(sources, crops)):
        u8 = veval.imread_rgb_uint8(src)[top:top + h, left:left + w]
        assert u8.shape == (h, w, 3)
        path = os.path.join(tmp, f"crop_{i}.png")
        Image.fromarray(u8).save(path)
        files.append(path)
        out[f"u8_{i}"] = np.ascontiguousarray(u8)
    ds = SimulateTest(files, seed=SEED)
    assert ds.noise.shape == (56, 56, 3) and ds.noise.dtype == np.float32 and ds.sigma_map.shape == (256, 256)
    out["files"] = np.asarray([os.path.basename(f) for f in files])
    out["noise"], out["sigma_map"] = ds.noise, ds.sigma_map
    for i in range(len(ds)):
        noisy, gt = ds[i]
        out[f"noisy_{i}"], out[f"gt_{i}"] = noisy.numpy(), gt.numpy()
        print(i, noisy.shape, noisy.dtype, float(noisy.mean()), float(gt.mean()))

path = os.path.join(HERE, "simulate_test.npz")
np.savez_compressed(path, **out)
print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")
