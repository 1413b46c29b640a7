"""Host-side checks of the device objective (virnet_amd/elbo.py, csrc/elbo.hip): the C ABI is bound at version 5, the kernels use no scratch,
the window taps restate the documented formula, argument errors are raised before any device work, and the default paths of
``loss.elbo_denoising_simple`` do not load the module."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_kernel_resources import _remarks, _table
from virnet_amd import _native, loss

NEW_SYMBOLS = ("virnet_elbo_workspace_bytes", "virnet_elbo_value", "virnet_elbo_grad", "virnet_noise_estimate")


def test_new_symbols_bound_and_abi_version_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5


def test_elbo_kernels_use_no_scratch():
    """the compiler's own resource remarks, as tests/test_kernel_resources.py reads them: zero scratch, no spilled vector register"""
    rows = _table(_remarks("elbo"))
    names = {r["pretty"] for r in rows}
    assert {"elbo_finish_kernel", "noise_estimate_kernel"} <= names, names
    assert sum(n.startswith("void elbo_value_kernel<") for n in names) == 4 and sum(n.startswith("void elbo_grad_kernel<") for n in names) == 4, names
    for r in rows:
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r


def _taps_restated(k):
    """float64 restatement of what OpenCV documents for getGaussianKernel(k, sigma > 0), at the sigma of utils/util_denoising.py:30"""
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    g = np.array([np.exp(-((i - (k - 1) / 2.0) ** 2) / (2.0 * sigma ** 2)) for i in range(k)], dtype=np.float64)
    return g / g.sum()


@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 21, 31])
def test_taps_restate_the_documented_formula(k):
    from virnet_amd import elbo
    g = elbo.gaussian_taps(k)
    assert g.dtype == np.float64 and g.shape == (k,)
    assert np.abs(g - _taps_restated(k)).max() <= 1e-16 and abs(g.sum() - 1.0) <= 1e-15
    assert np.array_equal(g, g[::-1]) and g.argmax() == k // 2


def test_taps_of_seven_and_of_one():
    from virnet_amd import elbo
    g = elbo.gaussian_taps(7)                   # sigma = 0.3 * 2 + 0.8 = 1.4
    assert abs(g.sum() - 1.0) <= 1e-15 and np.array_equal(g, g[::-1])
    assert abs(g[3] / g[2] - np.exp(1.0 / (2 * 1.4 ** 2))) <= 1e-14
    # one tap: [1] by the normalisation, whatever sigma (0.5 here) is
    assert np.array_equal(elbo.gaussian_taps(1), np.array([1.0])) and np.array_equal(_taps_restated(1), np.array([1.0]))


class _NoLaunch:
    """stands in for the loaded library: any call into it is an error"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: argument errors must be raised before any device work")


@pytest.fixture
def no_device_work(monkeypatch):
    from virnet_amd import elbo
    monkeypatch.setattr(elbo._native, "load", lambda: _NoLaunch())
    return elbo


def _args():
    z = torch.zeros
    return dict(mu=z(2, 3, 8, 8), sigma_est=z(2, 1, 8, 8), im_noisy=z(2, 3, 8, 8), im_gt=z(2, 3, 8, 8), eps2=1e-6, alpha0=torch.tensor([24.5]),
                beta0=z(2, 1, 8, 8))


@pytest.mark.parametrize("case, exc", [("not_a_tensor", TypeError), ("dtype_mu", TypeError), ("dtype_sigma", TypeError), ("rank", ValueError),
                                       ("mu_shape", ValueError), ("sigma_channels", ValueError), ("beta0_channels", ValueError),
                                       ("beta0_size", ValueError), ("gt_shape", ValueError), ("eps2", ValueError), ("alpha0_shape", TypeError),
                                       ("alpha0_type", TypeError), ("alpha0_value", ValueError), ("list_entry", ValueError),
                                       ("empty_list", ValueError), ("cpu", RuntimeError)])
def test_elbo_argument_errors_before_device_work(no_device_work, case, exc):
    elbo = no_device_work
    a = _args()
    z = torch.zeros
    if case == "not_a_tensor":
        a["im_gt"] = np.zeros((2, 3, 8, 8), dtype=np.float32)
    elif case == "dtype_mu":
        a["mu"] = a["mu"].double()
    elif case == "dtype_sigma":
        a["sigma_est"] = a["sigma_est"].half()
    elif case == "rank":
        a["im_noisy"] = z(3, 8, 8)
    elif case == "mu_shape":
        a["mu"] = z(2, 3, 8, 9)
    elif case == "sigma_channels":
        a["sigma_est"] = z(2, 2, 8, 8)
    elif case == "beta0_channels":
        a["beta0"] = z(2, 2, 8, 8)
    elif case == "beta0_size":
        a["beta0"] = z(2, 1, 4, 4)
    elif case == "gt_shape":
        a["im_gt"] = z(1, 3, 8, 8)
    elif case == "eps2":
        a["eps2"] = 0.0
    elif case == "alpha0_shape":
        a["alpha0"] = torch.tensor([24.5, 24.5])
    elif case == "alpha0_type":
        a["alpha0"] = "24.5"
    elif case == "alpha0_value":
        a["alpha0"] = 1.0
    elif case == "list_entry":
        a["mu"] = [z(2, 3, 8, 8), z(2, 3, 8, 9)]
    elif case == "empty_list":
        a["mu"] = []
    with pytest.raises(exc) as e:
        elbo.elbo_denoising(**a)
    if case == "cpu":
        assert "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("case, exc", [("even_k", ValueError), ("k33", ValueError), ("k0", ValueError), ("pad_ge_dim", ValueError),
                                       ("dtype", TypeError), ("shape", ValueError), ("rank", ValueError), ("cpu", RuntimeError)])
def test_noise_estimate_argument_errors_before_device_work(no_device_work, case, exc):
    elbo = no_device_work
    x, y, k = torch.zeros(2, 3, 40, 40), torch.zeros(2, 3, 40, 40), 7
    if case == "even_k":
        k = 6
    elif case == "k33":
        k = 33
    elif case == "k0":
        k = 0
    elif case == "pad_ge_dim":
        x, y = torch.zeros(2, 3, 40, 3), torch.zeros(2, 3, 40, 3)       # p = 3 is not < 3
    elif case == "dtype":
        y = y.double()
    elif case == "shape":
        y = torch.zeros(2, 3, 40, 41)
    elif case == "rank":
        x, y = torch.zeros(3, 40, 40), torch.zeros(3, 40, 40)
    with pytest.raises(exc) as e:
        elbo.noise_estimate(x, y, k)
    if case == "cpu":
        assert "no CPU fallback" in str(e.value)


def test_loss_keyword(no_device_work):
    a = _args()
    a["sigma_est"], a["beta0"] = a["sigma_est"] + 0.01, a["beta0"] + 0.2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.elbo_denoising_simple(**a, impl="hip")
    with pytest.raises(ValueError):
        loss.elbo_denoising_simple(**a, impl="bogus")
    assert len(loss.elbo_denoising_simple(**a)) == 4 and len(loss.elbo_denoising_simple(**a, impl="torch")) == 4      # CPU included


def test_c_abi_argument_errors_return_nonzero_with_a_message():
    """bad arguments never reach a launch: the entries return non-zero and set virnet_last_error (no device needed, pointers are never read)"""
    lib = _native.load()
    p = 4096                                           # any non-NULL, 16-byte aligned address: rejected calls do not touch it

    def value(ptrs=(p,) * 7, eps2=1e-6, ws=p, out=p, dims=(2, 3, 1, 1, 8, 8)):
        return lib.virnet_elbo_value(*ptrs, eps2, 1, ws, out, *dims, None)

    def grad(ptrs=(p,) * 7, eps2=1e-6, outs=(p, p), dims=(2, 3, 1, 1, 8, 8)):
        return lib.virnet_elbo_grad(*ptrs, eps2, 1.0, 1.0, *outs, *dims, None)
    for dims, word in [((2, 3, 2, 1, 8, 8), "sigma_est has 2 channels"), ((2, 3, 1, 2, 8, 8), "beta0 has 2 channels"), ((0, 3, 1, 1, 8, 8), "positive"),
                       ((2, 3, 1, 1, 0, 8), "positive"), ((2, 0, 1, 1, 8, 8), "positive"), ((2, 3, 1, 1, -8, 8), "positive"),
                       ((40000, 3, 1, 1, 256, 256), "2^31")]:
        assert value(dims=dims) != 0 and word in lib.virnet_last_error().decode()
        assert grad(dims=dims) != 0 and word in lib.virnet_last_error().decode()
        assert lib.virnet_elbo_workspace_bytes(dims[0], dims[1], dims[4], dims[5]) == 0 or "channels" in word
    for i in range(7):
        ptrs = tuple(0 if j == i else p for j in range(7))
        assert value(ptrs=ptrs) != 0 and "NULL" in lib.virnet_last_error().decode()
        assert grad(ptrs=ptrs) != 0 and "NULL" in lib.virnet_last_error().decode()
    assert value(ws=0) != 0 and value(out=0) != 0 and grad(outs=(0, p)) != 0 and grad(outs=(p, 0)) != 0
    assert value(eps2=0.0) != 0 and "eps2" in lib.virnet_last_error().decode()
    assert value(ptrs=(p + 2,) + (p,) * 6) != 0 and "misaligned" in lib.virnet_last_error().decode()
    for args, word in [((2, 3, 40, 40, 6), "window size"), ((2, 3, 40, 40, 33), "window size"), ((2, 3, 40, 40, 0), "window size"),
                       ((2, 3, 40, 3, 7), "does not fit"), ((0, 3, 40, 40, 7), "n*c"), ((2, 3, 0, 40, 7), "image")]:
        assert lib.virnet_noise_estimate(p, p, p, p, *args, 1e-10, None) != 0
        assert word in lib.virnet_last_error().decode()
    assert lib.virnet_noise_estimate(p, 0, p, p, 2, 3, 40, 40, 7, 1e-10, None) != 0 and "NULL" in lib.virnet_last_error().decode()
    # one fp64 (lh, kl_gauss, kl_Igamma) partial per workgroup of 256 items, 1024 workgroups at most
    assert lib.virnet_elbo_workspace_bytes(1, 1, 1, 1) == 24 and lib.virnet_elbo_workspace_bytes(2, 3, 17, 19) == 3 * 24
    assert lib.virnet_elbo_workspace_bytes(32, 3, 256, 256) == 1024 * 24


def test_default_paths_do_not_import_elbo():
    """elbo_denoising_simple with its default and with impl="torch" runs without virnet_amd.elbo ever being imported (a fresh interpreter)"""
    code = r"""
import sys
import torch
sys.path.insert(0, {repo!r})
from virnet_amd import loss
g = torch.Generator().manual_seed(0)
mu = torch.rand(2, 3, 8, 8, generator=g, requires_grad=True)
sigma = (torch.rand(2, 1, 8, 8, generator=g) * 0.05 + 1e-3).requires_grad_(True)
noisy, gt = torch.rand(2, 3, 8, 8, generator=g), torch.rand(2, 3, 8, 8, generator=g)
alpha0 = torch.tensor([24.5])
for kw in ({{}}, {{"impl": "torch"}}):
    out = loss.elbo_denoising_simple(mu, sigma, noisy, gt, 1e-6, alpha0, alpha0 * 0.01 * torch.ones(2, 1, 8, 8), **kw)
    out[0].backward()
import virnet_amd.train, virnet_amd.networks
assert "virnet_amd.elbo" not in sys.modules, "a default path imported virnet_amd.elbo"
print("ok")
""".format(repo=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
