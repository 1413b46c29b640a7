"""Host-side checks of the device degradation (virnet_amd/degrade.py, csrc/degrade.hip): the C ABI is bound at version 5, the one tap-table
helper reproduces both earlier constructions of the antialiased cubic, argument errors are raised before any device work, and the default
paths of the callers do not load the module."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_kernel_resources import _remarks, _table
from virnet_amd import _native, loss, sisr_eval

NEW_SYMBOLS = ("virnet_degrade_forward", "virnet_degrade_grad_image", "virnet_degrade_grad_kernel_workspace_bytes",
               "virnet_degrade_grad_kernel", "virnet_resample_axis")


def test_new_symbols_bound_and_abi_version_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5


def test_degrade_kernels_use_no_scratch():
    """the compiler's own resource remarks, as tests/test_kernel_resources.py reads them: zero scratch, no spilled vector register"""
    rows = _table(_remarks("degrade"))
    names = {r["pretty"] for r in rows}
    assert {"degrade_gx_kernel", "degrade_gk_kernel", "degrade_gk_finish"} <= names, names
    assert sum(n.startswith("void degrade_fwd_kernel<") for n in names) == 4 and sum(n.startswith("void resample_kernel<") for n in names) == 2, names
    for r in rows:
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r


def _old_resample_axis0(x, scale, n_out):
    """sisr_eval._resample_axis0 as it stood before the tap construction was factored out (the pinned restatement of ResizeRight)."""
    n_in = x.shape[0]
    eps = float(np.finfo(np.float32).eps)
    support = 4.0 / scale if scale < 1.0 else 4.0
    pos = np.arange(n_out) / scale + (n_in - 1) / 2 - (n_out - 1) / (2 * scale)
    left = np.ceil(pos - support / 2 - eps).astype(np.int64)
    taps = left[:, None] + np.arange(math.ceil(support - eps))
    mirror = np.concatenate([np.arange(n_in), np.arange(n_in - 1, -1, -1)])
    idx = mirror[np.remainder(taps, 2 * n_in)]
    d = pos[:, None] - idx
    wgt = scale * sisr_eval._cubic(scale * d) if scale < 1.0 else sisr_eval._cubic(d)
    tot = wgt.sum(1, keepdims=True)
    tot[tot == 0] = 1
    wgt = wgt / tot
    return (x[idx] * wgt.reshape(wgt.shape + (1,) * (x.ndim - 1))).sum(1)


@pytest.mark.parametrize("n_in", [12, 47, 64])
@pytest.mark.parametrize("sf", [2, 3, 4])
def test_tap_table_reproduces_both_constructions(n_in, sf):
    from virnet_amd import degrade
    idx, wgt = degrade.tap_table(n_in, sf)
    n_out = math.ceil(n_in / sf)
    assert idx.dtype == np.int32 and wgt.dtype == np.float64 and idx.shape == wgt.shape and idx.shape[0] == n_out
    assert idx.min() >= 0 and idx.max() < n_in
    dense = degrade.densify(idx, wgt, n_in)
    eye = np.eye(n_in)
    assert np.abs(dense - sisr_eval._resample_axis0(eye, 1.0 / sf, n_out)).max() <= 1e-15
    assert np.abs(dense - _old_resample_axis0(eye, 1.0 / sf, n_out)).max() <= 1e-15
    assert np.abs(dense - loss._bicubic_matrix(n_in, sf, "cpu", torch.float64).numpy()).max() <= 1e-15
    assert np.abs(dense.sum(1) - 1.0).max() <= 1e-14


@pytest.mark.parametrize("n_in", [12, 47, 64])
@pytest.mark.parametrize("sf", [2, 3, 4])
def test_transposed_table_densifies_to_the_transpose(n_in, sf):
    from virnet_amd import degrade
    idx, wgt = degrade.tap_table(n_in, sf)
    idx_t, wgt_t = degrade.transpose_taps(idx, wgt, n_in)
    assert idx_t.dtype == np.int32 and wgt_t.dtype == np.float64 and idx_t.shape == wgt_t.shape and idx_t.shape[0] == n_in
    assert idx_t.min() >= 0 and idx_t.max() < idx.shape[0]
    assert np.abs(degrade.densify(idx_t, wgt_t, idx.shape[0]) - degrade.densify(idx, wgt, n_in).T).max() <= 1e-15


def test_bicubic_downscale_is_unchanged_by_the_shared_helper():
    g = np.random.default_rng(3)
    im = g.random((23, 31, 3)).astype(np.float32)
    for sf in (2, 3, 4):
        want = _old_resample_axis0(im, 1.0 / sf, math.ceil(23 / sf))
        want = np.swapaxes(_old_resample_axis0(np.swapaxes(want, 0, 1), 1.0 / sf, math.ceil(31 / sf)), 0, 1)
        assert np.array_equal(sisr_eval.bicubic_downscale(im, sf), want)


class _NoLaunch:
    """stands in for the loaded library: any call into it is an error"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: argument errors must be raised before any device work")


@pytest.fixture
def no_device_work(monkeypatch):
    from virnet_amd import degrade
    monkeypatch.setattr(degrade._native, "load", lambda: _NoLaunch())
    return degrade


@pytest.mark.parametrize("case, exc", [("even_k", ValueError), ("k27", ValueError), ("sf5", ValueError), ("sf0", ValueError),
                                       ("pad_ge_dim", ValueError), ("dtype_image", TypeError), ("dtype_kernel", TypeError),
                                       ("batch", ValueError), ("kernel_shape", ValueError), ("downsampler", ValueError),
                                       ("border", ValueError), ("cpu", RuntimeError)])
def test_argument_errors_before_device_work(no_device_work, case, exc):
    degrade = no_device_work
    x, k, sf, kw = torch.zeros(2, 3, 32, 32), torch.zeros(2, 1, 21, 21), 4, {}
    if case == "even_k":
        k = torch.zeros(2, 1, 20, 20)
    elif case == "k27":
        x, k = torch.zeros(2, 3, 64, 64), torch.zeros(2, 1, 27, 27)
    elif case == "sf5":
        sf = 5
    elif case == "sf0":
        sf = 0
    elif case == "pad_ge_dim":
        x = torch.zeros(2, 3, 32, 10)           # p = 10 is not < 10
    elif case == "dtype_image":
        x = x.double()
    elif case == "dtype_kernel":
        k = k.half()
    elif case == "batch":
        k = torch.zeros(3, 1, 21, 21)
    elif case == "kernel_shape":
        k = torch.zeros(2, 3, 21, 21)
    elif case == "downsampler":
        kw["downsampler"] = "nearest"
    elif case == "border":
        kw["border"] = "zeros"
    with pytest.raises(exc) as e:
        degrade.blur_downsample(x, k, sf, **kw)
    if case == "cpu":
        assert "no CPU fallback" in str(e.value)


def test_cpu_tensors_raise_through_the_loss_keyword(no_device_work):
    x, k = torch.zeros(1, 3, 32, 32), torch.zeros(1, 1, 21, 21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.blur_downsample(x, k, 4, "direct", impl="hip")
    with pytest.raises(ValueError):
        loss.blur_downsample(x, k, 4, "direct", impl="triton")
    assert loss.blur_downsample(x, k, 4, "direct").shape == (1, 3, 8, 8)         # the default is the torch route, CPU included


def test_clip_with_a_gradient_is_refused(no_device_work):
    x, k = torch.zeros(1, 3, 32, 32, requires_grad=True), torch.zeros(1, 1, 5, 5)
    with pytest.raises(RuntimeError):                 # (CPU tensors: refused either way, before any launch)
        no_device_work.blur_downsample(x, k, 2, clip=True)
    with pytest.raises(TypeError):
        no_device_work.degrade_lr(np.zeros((32, 32, 3)), np.ones((21, 21)) / 441.0, 4)      # float64 image, as sisr_eval.degrade


def test_c_abi_argument_errors_return_nonzero_with_a_message():
    """bad sizes never reach a launch: the entries return non-zero and set virnet_last_error (no device needed, pointers are never read)"""
    lib = _native.load()
    p = 4096                                           # any non-NULL address: rejected calls do not touch it
    for args, word in [((2, 3, 64, 64, 20, 4, 0), "kernel size"), ((2, 3, 64, 64, 27, 4, 0), "kernel size"), ((2, 3, 64, 64, 21, 5, 0), "scale factor"),
                       ((2, 3, 64, 10, 21, 4, 0), "does not fit"), ((2, 3, 64, 64, 21, 4, 2), "border mode"), ((0, 3, 64, 64, 21, 4, 0), "n*c")]:
        assert lib.virnet_degrade_forward(p, p, p, *args, 0, None) != 0
        assert word in lib.virnet_last_error().decode()
        assert lib.virnet_degrade_grad_image(p, p, p, *args, None) != 0
        assert lib.virnet_degrade_grad_kernel(p, p, p, p, *args, None) != 0
        assert lib.virnet_degrade_grad_kernel_workspace_bytes(*args[:6]) == 0 or word == "border mode"
    assert lib.virnet_degrade_forward(0, p, p, 2, 3, 64, 64, 21, 4, 0, 0, None) != 0 and "NULL" in lib.virnet_last_error().decode()
    assert lib.virnet_resample_axis(p, 0, p, 0, p, p, 8, 6, 64, 16, 64, None) != 0          # fp32 -> fp32 is not offered
    assert lib.virnet_resample_axis(p, 0, p * 2, 1, p, p, 0, 6, 64, 16, 64, None) != 0 and "taps" in lib.virnet_last_error().decode()
    # 2 x 3 x 256 x 256, k = 21: 8 x 16 tiles of 16 x 32 blurred pixels at sf = 1, one fp32 partial per tap, tile and sample
    assert lib.virnet_degrade_grad_kernel_workspace_bytes(2, 3, 256, 256, 21, 1) == 2 * 16 * 8 * 441 * 4
    assert lib.virnet_degrade_grad_kernel_workspace_bytes(2, 3, 256, 256, 21, 4) == 2 * 4 * 2 * 441 * 4


def test_default_paths_do_not_import_degrade(tmp_path):
    """elbo_sisr and sisr_table with their defaults run without virnet_amd.degrade ever being imported (a fresh interpreter)."""
    code = r"""
import sys, os, glob, shutil
import numpy as np, torch
sys.path.insert(0, {repo!r})
from virnet_amd import loss, sisr_eval
g = torch.Generator().manual_seed(0)
n, sf = 2, 2
mu = torch.rand(n, 3, 24, 24, generator=g, requires_grad=True)
kinfo = torch.tensor([[1.0, 2.0, 0.1], [2.0, 1.0, -0.2]], requires_grad=True)
out, _ = loss.elbo_sisr(mu=mu, sigma_est=torch.full((n, 1, 1, 1), 1e-3), kinfo_est=kinfo, im_hr=torch.rand(n, 3, 24, 24, generator=g),
                        im_lr=torch.rand(n, 3, 12, 12, generator=g), sigma_prior=torch.full((n, 1, 1, 1), 1e-3), alpha0=torch.tensor([24.5]),
                        kinfo_gt=kinfo.detach(), kappa0=torch.tensor([50.0]), r2=1e-2, eps2=1e-6, sf=sf, k_size=9, penalty_K=[0.02, 2.0],
                        shift=False, downsampler="Bicubic")
out.backward()
dst = {tmp!r}
for f in sorted(glob.glob(os.path.join({repo!r}, "tests", "golden", "set5", "*.bmp")))[:1]:
    shutil.copy(f, dst)
rows = sisr_eval.sisr_table(lambda lr, s: np.repeat(np.repeat(lr, s, 0), s, 1), [dst + ":bmp"], 4, kernels=sisr_eval.test_kernels(4)[:1],
                            with_ssim=False)
assert len(rows) == 1 and isinstance(rows[0]["per_image_psnr_y"][0], float)
assert "virnet_amd.degrade" not in sys.modules, "a default path imported virnet_amd.degrade"
print("ok")
""".format(repo=REPO, tmp=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
