"""Host-side checks of the device SISR objective (virnet_amd/elbo.py ``elbo_sisr``, csrc/elbo_sisr.hip): the C ABI is bound at version 5, the
kernels use no scratch, argument errors are raised before any device work, the C entries refuse bad sizes and null pointers, the default
path of ``loss.elbo_sisr`` does not load the module, and the float64 composition that tests/test_elbo_sisr_gpu.py uses as its reference
reproduces the reference's golden values."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_kernel_resources import _remarks, _table
from virnet_amd import _native, loss

GOLDEN = os.path.join(REPO, "tests", "golden")
NEW_SYMBOLS = ("virnet_sisr_head_workspace_bytes", "virnet_sisr_head_forward", "virnet_sisr_head_backward", "virnet_sisr_hr_workspace_bytes",
               "virnet_sisr_hr_value", "virnet_sisr_hr_grad", "virnet_sisr_lr_workspace_bytes", "virnet_sisr_lr_value", "virnet_sisr_lr_grad",
               "virnet_sisr_finish")


def test_new_symbols_bound_and_abi_version_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5


def test_elbo_sisr_kernels_use_no_scratch():
    """the compiler's own resource remarks, as tests/test_kernel_resources.py reads them: zero scratch, no spilled vector register"""
    rows = _table(_remarks("elbo_sisr"))
    names = {r["pretty"] for r in rows}
    assert {"sisr_head_fwd_kernel", "sisr_head_bwd_kernel", "sisr_head_finish_kernel", "sisr_hr_finish_kernel", "sisr_lr_finish_kernel",
            "sisr_sum_kernel"} <= names, names
    for stem in ("sisr_hr_value_kernel", "sisr_hr_grad_kernel", "sisr_lr_value_kernel", "sisr_lr_grad_kernel"):
        assert sum(n.startswith(f"void {stem}<") for n in names) == 2, (stem, names)
    for r in rows:
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r


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
    return dict(mu=z(2, 3, 16, 24), sigma_est=z(2, 1, 1, 1), kinfo_est=z(2, 3), im_hr=z(2, 3, 16, 24), im_lr=z(2, 3, 8, 12), sigma_prior=z(2, 1, 1, 1),
                alpha0=torch.tensor([24.5]), kinfo_gt=z(2, 3), kappa0=torch.tensor([50.0]), r2=1e-4, eps2=1e-5, sf=2, k_size=9, penalty_K=[0.02, 2.0],
                shift=False, downsampler="Direct")


CASES = [("not_a_tensor", TypeError), ("dtype_mu", TypeError), ("dtype_kinfo", TypeError), ("rank_mu", ValueError), ("rank_sigma", ValueError),
         ("hr_shape", ValueError), ("kinfo_shape", ValueError), ("kinfo_gt_shape", ValueError), ("lr_shape", ValueError), ("lr_shape_ceil", ValueError),
         ("sigma_shape", ValueError), ("prior_shape", ValueError), ("pad_ge_dim", ValueError), ("k26", ValueError), ("k0", ValueError),
         ("even_k_hip", ValueError), ("sf0", ValueError), ("sf5", ValueError), ("sf_float", ValueError), ("eps2", ValueError), ("r2", ValueError),
         ("alpha0_value", ValueError), ("alpha0_shape", TypeError), ("alpha0_type", TypeError), ("kappa0_value", ValueError),
         ("kappa0_shape", TypeError), ("kappa0_type", TypeError), ("penalty_len", ValueError), ("penalty_nan", ValueError), ("penalty_type", TypeError),
         ("downsampler", ValueError), ("degrade_impl", ValueError), ("draws_len", TypeError), ("draws_shape", ValueError), ("draws_dtype", TypeError),
         ("cpu", RuntimeError)]


@pytest.mark.parametrize("case, exc", CASES)
def test_elbo_sisr_argument_errors_before_device_work(no_device_work, case, exc):
    elbo = no_device_work
    a = _args()
    z = torch.zeros
    kw = {}
    if case == "not_a_tensor":
        a["im_hr"] = np.zeros((2, 3, 16, 24), dtype=np.float32)
    elif case == "dtype_mu":
        a["mu"] = a["mu"].double()
    elif case == "dtype_kinfo":
        a["kinfo_est"] = a["kinfo_est"].double()
    elif case == "rank_mu":
        a["mu"] = z(3, 16, 24)
    elif case == "rank_sigma":
        a["sigma_est"] = z(2, 1)
    elif case == "hr_shape":
        a["im_hr"] = z(2, 3, 16, 25)
    elif case == "kinfo_shape":
        a["kinfo_est"] = z(2, 2)
    elif case == "kinfo_gt_shape":
        a["kinfo_gt"] = z(3, 3)
    elif case == "lr_shape":
        a["im_lr"] = z(2, 3, 8, 11)
    elif case == "lr_shape_ceil":                      # 15 x 23 at sf 2 degrades to 8 x 12, not 7 x 11
        a["mu"], a["im_hr"], a["im_lr"] = z(2, 3, 15, 23), z(2, 3, 15, 23), z(2, 3, 7, 11)
    elif case == "sigma_shape":
        a["sigma_est"] = z(2, 2, 8, 12)
    elif case == "prior_shape":
        a["sigma_prior"] = z(2, 1, 16, 24)
    elif case == "pad_ge_dim":
        a["mu"], a["im_hr"], a["im_lr"] = z(2, 3, 4, 24), z(2, 3, 4, 24), z(2, 3, 2, 12)       # 9 // 2 = 4 is not < 4
    elif case == "k26":
        a["k_size"] = 27
    elif case == "k0":
        a["k_size"] = 0
    elif case == "even_k_hip":
        a["k_size"] = 8
    elif case == "sf0":
        a["sf"] = 0
    elif case == "sf5":
        a["sf"] = 5
    elif case == "sf_float":
        a["sf"] = 2.0
    elif case == "eps2":
        a["eps2"] = 0.0
    elif case == "r2":
        a["r2"] = -1e-4
    elif case == "alpha0_value":
        a["alpha0"] = 1.0
    elif case == "alpha0_shape":
        a["alpha0"] = torch.tensor([24.5, 24.5])
    elif case == "alpha0_type":
        a["alpha0"] = "24.5"
    elif case == "kappa0_value":
        a["kappa0"] = 0.5
    elif case == "kappa0_shape":
        a["kappa0"] = torch.tensor([50.0]).double()
    elif case == "kappa0_type":
        a["kappa0"] = None
    elif case == "penalty_len":
        a["penalty_K"] = [0.02]
    elif case == "penalty_nan":
        a["penalty_K"] = [0.02, float("nan")]
    elif case == "penalty_type":
        a["penalty_K"] = 2.0
    elif case == "downsampler":
        a["downsampler"] = "nearest"
    elif case == "degrade_impl":
        kw["degrade_impl"] = "fft"
    elif case == "draws_len":
        kw["draws"] = (z(2, 2), z(2, 1))
    elif case == "draws_shape":
        kw["draws"] = (z(2, 2), z(2), z(2, 3, 16, 24))
    elif case == "draws_dtype":
        kw["draws"] = (z(2, 2), z(2, 1), z(2, 3, 16, 24).double())
    with pytest.raises(exc) as e:
        elbo.elbo_sisr(**a, **kw)
    if case == "cpu":
        assert "no CPU fallback" in str(e.value)


def test_loss_keyword(no_device_work):
    a = _args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.elbo_sisr(**a, impl="hip")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.elbo_sisr(**a, impl="hip", degrade_impl="hip")
    with pytest.raises(ValueError):
        loss.elbo_sisr(**a, impl="bogus")


def test_c_abi_argument_errors_return_nonzero_with_a_message():
    """bad arguments never reach a launch: the entries return non-zero and set virnet_last_error (no device needed, pointers are never read)"""
    lib = _native.load()
    p = 4096                                           # any non-NULL, 16-byte aligned address: rejected calls do not touch it

    def err():
        return lib.virnet_last_error().decode()

    def head_f(ptrs=(p,) * 5, sc=(1e-4, 0.02, 2.0), ks=(9, 2, 0), outs=(p, p, p), n=2):
        return lib.virnet_sisr_head_forward(*ptrs, *sc, *ks, *outs, n, None)

    def head_b(ptrs=(p,) * 7, sc=(1e-4, 0.02, 2.0), ks=(9, 2, 0), out=p, n=2):
        return lib.virnet_sisr_head_backward(*ptrs, *sc, *ks, out, n, None)
    for kw, word in [(dict(n=0), "batch size"), (dict(ks=(26, 2, 0)), "kernel size"), (dict(ks=(0, 2, 0)), "kernel size"), (dict(ks=(9, 5, 0)), "scale factor"),
                     (dict(ks=(9, 0, 0)), "scale factor"), (dict(sc=(0.0, 0.02, 2.0)), "r2"), (dict(sc=(1e-4, float("inf"), 2.0)), "penalty_K")]:
        assert head_f(**kw) != 0 and word in err()
        assert head_b(**kw) != 0 and word in err()
    for i in range(5):
        assert head_f(ptrs=tuple(0 if j == i else p for j in range(5))) != 0 and "NULL" in err()
    for i in range(7):
        assert head_b(ptrs=tuple(0 if j == i else p for j in range(7))) != 0 and "NULL" in err()
    assert head_f(outs=(0, p, p)) != 0 and head_f(outs=(p, 0, p)) != 0 and head_f(outs=(p, p, 0)) != 0 and head_b(out=0) != 0
    assert head_f(ptrs=(p + 2,) + (p,) * 4) != 0 and "misaligned" in err()
    assert lib.virnet_sisr_head_workspace_bytes(0) == 0 and lib.virnet_sisr_head_workspace_bytes(5) == 5 * 3 * 8

    def hr_v(ptrs=(p,) * 3, eps2=1e-5, outs=(p, p, p), dims=(2, 3, 8, 8)):
        return lib.virnet_sisr_hr_value(*ptrs, eps2, *outs, *dims, None)

    def hr_g(ptrs=(p,) * 4, eps2=1e-5, out=p, dims=(2, 3, 8, 8)):
        return lib.virnet_sisr_hr_grad(*ptrs, eps2, out, *dims, None)
    for dims, word in [((0, 3, 8, 8), "positive"), ((2, 0, 8, 8), "positive"), ((2, 3, -8, 8), "positive"), ((2, 3, 8, 0), "positive"),
                       ((4000, 3, 512, 512), "2^31")]:
        assert hr_v(dims=dims) != 0 and word in err()
        assert hr_g(dims=dims) != 0 and word in err()
        assert lib.virnet_sisr_hr_workspace_bytes(*dims) == 0 and lib.virnet_sisr_lr_workspace_bytes(*dims) == 0
    for i in range(3):
        assert hr_v(ptrs=tuple(0 if j == i else p for j in range(3))) != 0 and "NULL" in err()
    for i in range(4):
        assert hr_g(ptrs=tuple(0 if j == i else p for j in range(4))) != 0 and "NULL" in err()
    assert hr_v(outs=(0, p, p)) != 0 and hr_v(outs=(p, 0, p)) != 0 and hr_v(outs=(p, p, 0)) != 0 and hr_g(out=0) != 0
    assert hr_v(eps2=0.0) != 0 and "eps2" in err() and hr_g(eps2=-1.0) != 0 and "eps2" in err()
    assert hr_v(ptrs=(p + 2, p, p)) != 0 and "misaligned" in err()
    # one fp64 partial per workgroup of 256 items, 1024 workgroups at most
    assert lib.virnet_sisr_hr_workspace_bytes(1, 1, 1, 1) == 8 and lib.virnet_sisr_hr_workspace_bytes(2, 3, 17, 19) == 8 * 8
    assert lib.virnet_sisr_hr_workspace_bytes(16, 3, 256, 256) == 1024 * 8

    def lr_v(ptrs=(p,) * 9, dims=(2, 3, 8, 8), lay=(1, 0, 1, 0)):
        return lib.virnet_sisr_lr_value(*ptrs, *dims, *lay, None)

    def lr_g(ptrs=(p,) * 10, dims=(2, 3, 8, 8), lay=(1, 0, 1, 0)):
        return lib.virnet_sisr_lr_grad(*ptrs, *dims, *lay, None)
    for kw, word in [(dict(dims=(0, 3, 8, 8)), "positive"), (dict(dims=(2, 3, 8, 0)), "positive"), (dict(dims=(70000, 1, 8, 8)), "65535"),
                     (dict(lay=(2, 1, 1, 0)), "sigma_est has 2 channels"), (dict(lay=(3, 0, 1, 0)), "sigma_est has 3 channels"),
                     (dict(lay=(1, 1, 2, 1)), "sigma_prior has 2 channels"), (dict(lay=(1, 1, 3, 0)), "sigma_prior has 3 channels")]:
        assert lr_v(**kw) != 0 and word in err()
        assert lr_g(**kw) != 0 and word in err()
    for i in range(9):
        assert lr_v(ptrs=tuple(0 if j == i else p for j in range(9))) != 0 and "NULL" in err()
    for i in range(10):
        assert lr_g(ptrs=tuple(0 if j == i else p for j in range(10))) != 0 and "NULL" in err()
    assert lr_v(ptrs=(p + 2,) + (p,) * 8) != 0 and "misaligned" in err()
    # [n][workgroups per sample][4] fp64, 256 workgroups per sample at most
    assert lib.virnet_sisr_lr_workspace_bytes(2, 3, 9, 11) == 2 * 1 * 32 and lib.virnet_sisr_lr_workspace_bytes(1, 3, 297, 295) == 256 * 32
    for i in range(5):
        assert lib.virnet_sisr_finish(*(0 if j == i else p for j in range(5)), None) != 0 and "NULL" in err()


def test_default_path_does_not_import_elbo():
    """elbo_sisr with its defaults and with impl="torch" runs without virnet_amd.elbo ever being imported (a fresh interpreter)"""
    code = r"""
import sys
import torch
sys.path.insert(0, {repo!r})
from virnet_amd import loss
g = torch.Generator().manual_seed(0)
mu = torch.rand(2, 3, 18, 22, generator=g, requires_grad=True)
sigma = (torch.rand(2, 1, 1, 1, generator=g) * 0.01 + 1e-4).requires_grad_(True)
kinfo = torch.tensor([[1.2, 0.8, 0.1], [2.0, 1.5, -0.3]], requires_grad=True)
hr, lr = torch.rand(2, 3, 18, 22, generator=g), torch.rand(2, 3, 9, 11, generator=g)
for kw in ({{}}, {{"impl": "torch"}}):
    out, parts = loss.elbo_sisr(mu, sigma, kinfo, hr, lr, sigma.detach() * 1.1, torch.tensor([24.5]), kinfo.detach() * 1.1, torch.tensor([50.0]), 1e-4, 1e-5,
                                2, 9, [0.02, 2.0], False, "Direct", **kw)
    out.backward()
    assert len(parts) == 8
import virnet_amd.train, virnet_amd.networks
assert "virnet_amd.elbo" not in sys.modules, "a default path imported virnet_amd.elbo"
print("ok")
""".format(repo=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


@pytest.mark.parametrize("down", ["Bicubic", "Direct"])
def test_reference_composition_reproduces_the_golden(down):
    """the composition of loss.py's public pieces that tests/test_elbo_sisr_gpu.py evaluates in float64, here in fp32 with the draws torch
    makes from ``torch_seed``: the bars of tests/test_loss.py::test_elbo_sisr_matches_reference_golden"""
    from sisr_objective_ref import golden_inputs, composition
    from virnet_amd import elbo  # noqa: F401  (the composition documents virnet_amd.elbo.elbo_sisr: the module must exist)
    G = json.load(open(os.path.join(GOLDEN, "loss_sisr.json")))
    if G["torch_version"] != torch.__version__:
        pytest.skip(f"golden drawn with torch {G['torch_version']}, this is {torch.__version__}: the random streams may differ")
    c = G["cases"][down]
    t = golden_inputs(G)
    for k in ("mu", "sigma_est", "kinfo_est"):
        t[k].requires_grad_(True)
    torch.manual_seed(G["torch_seed"])
    conc = torch.ones_like(t["kinfo_est"][:, :2].detach()) * (t["kappa0"] - 1)
    gamma = torch._standard_gamma(conc).clamp_(min=torch.finfo(torch.float32).tiny)
    rho_eps = torch.randn_like(t["kinfo_est"].detach()[:, 2].unsqueeze(1))
    z_eps = torch.randn_like(t["mu"])
    out = composition(t, (gamma, rho_eps, z_eps), downsampler=down)
    out["loss"].backward()
    got = [float(out[k].detach()) for k in ("loss", "lh", "kl_rnet", "kl_snet", "kl_knet", "kl_k0", "kl_k1", "kl_k2")]
    assert got == pytest.approx(c["values"], rel=2e-5)
    ker = out["kernel"].detach()
    assert float(ker.double().sum()) == pytest.approx(c["kernel_sum"], rel=1e-6) and float(ker.max()) == pytest.approx(c["kernel_max"], rel=1e-5)
    assert [float(ker[0, 0, 4, 4]), float(ker[1, 0, 3, 5])] == pytest.approx(c["kernel_00"], rel=1e-5)
    mu, sigma, kinfo = t["mu"], t["sigma_est"], t["kinfo_est"]
    assert float(mu.grad.double().sum()) == pytest.approx(c["dmu_sum"], rel=1e-4) and float(mu.grad.abs().max()) == pytest.approx(c["dmu_absmax"], rel=1e-4)
    assert [float(v) for v in sigma.grad.reshape(-1)] == pytest.approx(c["dsigma"], rel=1e-4)
    assert [float(v) for v in kinfo.grad.reshape(-1)] == pytest.approx(c["dkinfo"], rel=2e-3, abs=1e-4)
