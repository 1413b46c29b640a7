#!/usr/bin/env python
"""Golden mix for virnet_amd/datagen.py (mixup_np, mixup, real_batch), produced by the REFERENCE's own ``MixUp_AUG.aug``
(datasets/data_tools.py:12-30) on the CPU.

Build container only: imports the reference (its checkout named by VIRNET_REFERENCE) at generation time; no test reads it.  cv2, skimage,
h5py and lmdb are not installed there and are stubbed (``aug`` uses none of them; they are imported at the top of the reference's modules).
``aug`` moves ``lam`` to the GPU with ``.cuda()``: ``Tensor.cuda`` is patched to the identity for the call, so the arithmetic is the
reference's expressions on torch's CPU fp32 kernels.

Writes tests/golden/mixup.npz:
  * ``seed``          what ``torch.manual_seed`` received right before ``aug``
  * ``gt``, ``noisy`` the two inputs, fp32 [9,3,20,20], each ``u8 * fp32(1/255)`` of seeded uint8 values
  * ``perm``, ``lam`` ``torch.randperm(9)`` and the Beta(0.6, 0.6) ``rsample((9, 1))``, re-drawn from the same seed in ``aug``'s order
  * ``out_gt``, ``out_noisy``  what ``aug(gt, noisy)`` returned
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VIRNET_REFERENCE")
if not REF or not os.path.isdir(REF):
    sys.exit("set VIRNET_REFERENCE to a checkout of the reference")
sys.path.insert(0, REF)

for name in ("cv2", "skimage", "h5py", "lmdb"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["skimage"].img_as_ubyte = None
sys.modules["skimage"].img_as_float32 = None

from datasets.data_tools import MixUp_AUG  # noqa: E402  (the reference)

SEED, N, C, P = 11, 9, 3, 20
g = np.random.default_rng(SEED)
gt, noisy = (g.integers(0, 256, (N, C, P, P), dtype=np.uint8).astype(np.float32) * np.float32(1.0 / 255.0) for _ in range(2))

mixer = MixUp_AUG()
real_cuda = torch.Tensor.cuda
torch.Tensor.cuda = lambda self, *a, **k: self
try:
    torch.manual_seed(SEED)
    out_gt, out_noisy = mixer.aug(torch.from_numpy(gt), torch.from_numpy(noisy))
finally:
    torch.Tensor.cuda = real_cuda

torch.manual_seed(SEED)
perm = torch.randperm(N)
lam = mixer.dist.rsample((N, 1)).view(-1)

out = dict(seed=np.asarray(SEED, dtype=np.int64), gt=gt, noisy=noisy, perm=perm.numpy().astype(np.int64), lam=lam.numpy().astype(np.float32),
           out_gt=out_gt.numpy(), out_noisy=out_noisy.numpy())
assert out["out_gt"].dtype == np.float32 and out["out_gt"].shape == (N, C, P, P)
path = os.path.join(HERE, "mixup.npz")
np.savez_compressed(path, **out)
print(f"{path}: {os.path.getsize(path)} bytes; perm {out['perm'].tolist()}, lam {out['lam'].tolist()}")
