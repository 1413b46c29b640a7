"""The device SISR objective (virnet_amd/elbo.py ``elbo_sisr``, csrc/elbo_sisr.hip) against float64 on the CPU.

Reference: tests/sisr_objective_ref.py -- ``loss.py``'s public pieces composed as ``loss.elbo_sisr`` composes them, on the same explicit
draws, evaluated on the fp32 inputs upcast to float64 with autograd for the gradients (tests/test_elbo_sisr_host.py anchors the composition
to the reference's golden values).  Bars (derived, not tuned), U = 8 * 2^-23 as in tests/test_elbo_gpu.py: a kernel tap is computed in fp64
and rounded once (2^-23 of itself); a mean or a gradient element formed from fp32 terms may differ by U times the sum of the absolute values
of its addends; ``lh`` additionally inherits the degradation's own per-element bar (tests/test_degrade_gpu.py: k^2 2^-23 sum |w| |zz|) through
(alpha0 - 1) / beta |x - y|.  The gradients of the whole objective, which pass through the degradation's adjoints, are held to at most four
times the error of the parent's fp32 torch composition on the device, and never above the bars of
tests/test_degrade_gpu.py::test_elbo_sisr_hip_against_torch_on_the_device."""
import functools
import json
import math
import os

import pytest
import torch

from conftest import REPO
from sisr_objective_ref import ALPHA0, EPS2, KAPPA0, PENALTY_K, R2, composition, covariance, golden_inputs, knet_terms, lr_terms
from virnet_amd import _native, loss

pytestmark = pytest.mark.gpu

U = 8.0 * 2.0 ** -23
EPS = 2.0 ** -23
GOLDEN = os.path.join(REPO, "tests", "golden")


def _elbo():
    from virnet_amd import elbo
    return elbo


# (N, sf, LR h, LR w, k, downsampler, sigma_est / sigma_prior layout): the golden's shape with both downsamplers and the three layouts
# ("s" [N,1,1,1], "p" [N,1,h,w], "c" [N,3,h,w]); an HR plane of 15 x 21 = 315 pixels (no multiple of four: scalar accesses); the training
# k and sf at the smallest image that allows k // 2 < 64; sf 1; LOOP: see test_loop_shape_takes_a_second_trip_and_many_partials
LOOP = (2, 1, 297, 295, 5, "Direct", "ss")
CASES = [(2, 2, 9, 11, 9, "Bicubic", "ss"), (2, 2, 9, 11, 9, "Direct", "ss"), (2, 2, 9, 11, 9, "Direct", "ps"), (2, 2, 9, 11, 9, "Bicubic", "cp"),
         (1, 3, 5, 7, 9, "Direct", "ss"), (2, 4, 16, 16, 21, "Bicubic", "ss"), (2, 4, 16, 16, 21, "Direct", "cp"), (1, 1, 12, 12, 5, "Direct", "ps"), LOOP]


def _sigma_shape(code, n, h, w):
    return {"s": (n, 1, 1, 1), "p": (n, 1, h, w), "c": (n, 3, h, w)}[code]


@functools.lru_cache(maxsize=None)
def make_inputs(case, seed=0):
    """fp32 CPU tensors of the family of tests/test_degrade_gpu.py::test_elbo_sisr_hip_against_torch_on_the_device, with explicit draws:
    lambda in [0.5, 3.5], |rho| <= 0.6, r2 = 1e-4, kappa0 = 50 -- the clamp is inactive and det >= 0.64 v1 v2 (asserted on the reference)"""
    n, sf, hl, wl, k, down, lay = case
    g = torch.Generator().manual_seed(2000 + seed)
    h, w = hl * sf, wl * sf

    def kinfo():
        return torch.cat([torch.rand(n, 2, generator=g) * 3 + 0.5, torch.rand(n, 1, generator=g) * 1.2 - 0.6], 1)
    t = dict(mu=torch.rand(n, 3, h, w, generator=g), sigma_est=torch.rand(_sigma_shape(lay[0], n, hl, wl), generator=g) * 0.01 + 1e-4,
             kinfo_est=kinfo(), im_hr=torch.rand(n, 3, h, w, generator=g), im_lr=torch.rand(n, 3, hl, wl, generator=g),
             sigma_prior=torch.rand(_sigma_shape(lay[1], n, hl, wl), generator=g) * 0.01 + 1e-4, kinfo_gt=kinfo(),
             alpha0=torch.tensor([ALPHA0]), kappa0=torch.tensor([KAPPA0]))
    gamma = torch._standard_gamma(torch.full((n, 2), KAPPA0 - 1), generator=g)
    draws = (gamma, torch.randn(n, 1, generator=g), torch.randn(n, 3, h, w, generator=g))
    t.update(r2=R2, eps2=EPS2, sf=sf, k_size=k, penalty_K=list(PENALTY_K), shift=False)
    return t, draws


def to(t, draws, device=None, dtype=None):
    def cv(v):
        return v.to(device=device, dtype=dtype) if isinstance(v, torch.Tensor) else v
    return {k: cv(v) for k, v in t.items()}, tuple(cv(d) for d in draws)


GRAD_KEYS = ("mu", "sigma_est", "kinfo_est")


def run_composition(case, device, dtype, seed=0):
    """values and gradients of the composition (upstream 1) in the given precision on the given device"""
    t, draws = to(*make_inputs(case, seed), device=device, dtype=dtype)
    for k in GRAD_KEYS:
        t[k] = t[k].clone().requires_grad_(True)
    out = composition(t, draws, case[5])
    grads = torch.autograd.grad(out["loss"], [t[k] for k in GRAD_KEYS])
    return t, draws, {k: v.detach() for k, v in out.items()}, dict(zip(GRAD_KEYS, grads))


def abs_degrade(zz, kernel, sf, down):
    """sum |w| |zz| per LR element: the degradation applied to absolute values with absolute taps (float64)"""
    if down.lower() == "direct":
        return loss.blur_downsample(zz.abs(), kernel.abs(), sf, "direct")
    blur = loss.blur_downsample(zz.abs(), kernel.abs(), 1, "direct")
    ah = loss._bicubic_matrix(zz.shape[-2], sf, blur.device, blur.dtype).abs()
    aw = loss._bicubic_matrix(zz.shape[-1], sf, blur.device, blur.dtype).abs()
    return ah @ blur @ aw.t()


@functools.lru_cache(maxsize=None)
def reference(case, seed=0):
    """float64 values, gradients and bars, computed once per case and left unchanged"""
    t, draws, out, grads = run_composition(case, "cpu", torch.float64, seed)
    n, sf, hl, wl, k, down, _ = case
    # the premises of the input family: a bad draw fails here instead of loosening a comparison
    assert float(out["rho_raw"].abs().max()) < 1.0, "the clamp is active"
    cov = out["cov"]
    det = cov[:, 0, 0, 0] * cov[:, 0, 1, 1] - cov[:, 0, 0, 1] ** 2
    assert bool((det >= 0.64 * cov[:, 0, 0, 0] * cov[:, 0, 1, 1] * (1 - 1e-12)).all()), "a covariance is close to singular"
    with torch.no_grad():
        a0, kap = t["alpha0"], t["kappa0"]
        a, ak = a0 - 1, kap - 1
        beta, beta0 = t["sigma_est"] * a0, t["sigma_prior"] * a0
        x, y = t["im_lr"], out["y"]
        bars = {}
        bars["kl_rnet"] = U * float(out["kl_rnet"])
        bars["kl_snet"] = U * float(((a * beta0 / beta).abs() + a.abs() + (a * beta.log()).abs() + (a * beta0.log()).abs()).mean())
        for i in (0, 1):
            bq, bp = kap * t["kinfo_est"][:, i], kap * t["kinfo_gt"][:, i]
            bars[f"kl_k{i}"] = U * float(((ak * bp / bq).abs() + ak.abs() + (ak * bq.log()).abs() + (ak * bp.log()).abs()).mean())
        bars["kl_k2"] = U * float(out["kl_k2"].abs())
        # kl_knet is an fp32 combination (two additions, a division, a product) of the three fp32 terms
        third = t["penalty_K"][1] / 3
        bars["kl_knet"] = (bars["kl_k0"] + bars["kl_k1"] + bars["kl_k2"]) * third + 4 * 2.0 ** -24 * float(out["kl_k0"].abs() + out["kl_k1"].abs() + out["kl_k2"].abs()) * third
        a_lh = float((0.5 * beta.log().abs() + 0.5 * torch.digamma(a).abs() + 0.5 * (a / beta) * (x - y) ** 2).mean()) + 0.5 * math.log(2 * math.pi)
        delta = k * k * EPS * abs_degrade(out["zz"], out["kernel"], sf, down)
        bars["lh"] = U * a_lh + float(((a / beta) * (x - y).abs() * delta).mean())
        bars["loss"] = bars["lh"] + bars["kl_rnet"] + bars["kl_snet"] + bars["kl_knet"] + 3 * 2.0 ** -24 * sum(abs(float(out[k_])) for k_ in ("lh", "kl_rnet", "kl_snet", "kl_knet"))
    return dict(t=t, draws=draws, out=out, grads=grads, bars=bars)


def run_hip(case, seed=0, degrade_impl="hip", scale=None, floats=False, backward=True, mutate=None):
    t, draws = to(*make_inputs(case, seed), device="cuda")
    if mutate is not None:
        mutate(t)
    for k in GRAD_KEYS:
        t[k] = t[k].clone().requires_grad_(True)
    if floats:
        t["alpha0"], t["kappa0"] = ALPHA0, KAPPA0
    total, parts = _elbo().elbo_sisr(downsampler=case[5], degrade_impl=degrade_impl, draws=draws, **t)
    if backward:
        (total if scale is None else scale * total).backward()
    return total, parts, {k: t[k].grad for k in GRAD_KEYS}


NAMES = ("lh", "kl_rnet", "kl_snet", "kl_knet", "kl_k0", "kl_k1", "kl_k2")


def check_values(total, parts, ref):
    out, bars = ref["out"], ref["bars"]
    pairs = [("loss", total)] + list(zip(NAMES, parts[:7]))
    for name, got in pairs:
        err = abs(float(got.detach().double()) - float(out[name]))
        print(f"{name}: {float(got):.9g} vs {float(out[name]):.12g}: |diff| {err:.3e}, bar {bars[name]:.3e} ({err / bars[name]:.3f} of it)")
    for name, got in pairs:
        assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda, name
        assert abs(float(got.detach().double()) - float(out[name])) <= bars[name], name
    kernel, want = parts[7], out["kernel"]
    assert kernel.shape == want.shape and kernel.dtype == torch.float32 and not kernel.requires_grad
    ratio = (kernel.cpu().double() - want).abs() / (EPS * want + 1e-37)
    print(f"kernel: worst tap at {float(ratio.max()):.3f} of 2^-23 of itself")
    assert float(ratio.max()) <= 1.0
    lh, rnet, snet, knet = parts[:4]
    assert float(total) == float(((lh + rnet) + snet) + knet)           # the fp32 sum of the parts, in the reference's order


def worst_ratio(got, want, bar):
    """max over the elements of |got - want| / bar; an element whose bar is zero (an addend that vanishes exactly, e.g. y == x) must be
    exact and counts as 0 then, as infinity otherwise"""
    err = (got.detach().cpu().double() - want).abs()
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


def rel_err(got, want):
    return float((got.detach().cpu().double() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("case", CASES)
def test_values_and_kernel_against_float64(case):
    total, parts, _ = run_hip(case, backward=False)
    check_values(total, parts, reference(case))


def test_torch_degradation_route_holds_the_same_bars():
    case = CASES[1]
    total, parts, _ = run_hip(case, degrade_impl="torch", backward=False)
    check_values(total, parts, reference(case))


def test_loop_shape_takes_a_second_trip_and_many_partials():
    """LOOP is chosen from the implementation's grid constants: an odd plane size (one item per element), in the HR passes more items than
    the largest grid has threads and more partials than the finishing workgroup is wide; in the LR passes more pixels per sample than a
    sample's workgroups have threads and, over the two samples, more partials than the finishing workgroup is wide."""
    elbo = _elbo()
    n, sf, hl, wl, _, _, _ = LOOP
    h, w = hl * sf, wl * sf
    lib = _native.load()
    assert (h * w) % 4 != 0 and n * 3 * h * w > elbo.SISR_MAX_BLOCKS * elbo.SISR_THREADS and elbo.SISR_MAX_BLOCKS > elbo.SISR_THREADS
    assert lib.virnet_sisr_hr_workspace_bytes(n, 3, h, w) == elbo.SISR_MAX_BLOCKS * 8
    assert (hl * wl) % 4 != 0 and hl * wl > elbo.SISR_LR_BLOCKS * elbo.SISR_THREADS and n * elbo.SISR_LR_BLOCKS > elbo.SISR_THREADS
    assert lib.virnet_sisr_lr_workspace_bytes(n, 3, hl, wl) == n * elbo.SISR_LR_BLOCKS * 4 * 8


# ---- the gradient passes alone: the stage Functions with a hand-made upstream -----------------------------------------------------------
STAGE_CASES = [CASES[0], CASES[2], CASES[3], CASES[4], CASES[6], LOOP]


@pytest.mark.parametrize("case", STAGE_CASES)
def test_hr_pass_zz_and_gradient(case):
    elbo = _elbo()
    ref = reference(case)
    t, draws = ref["t"], ref["draws"]
    mu32, hr32, z32 = (v.float().cuda() for v in (t["mu"], t["im_hr"], draws[2]))
    g = torch.Generator().manual_seed(7)
    gzz, gs = torch.randn(mu32.shape, generator=g) * 1e-3, torch.tensor(0.7)
    mu = mu32.clone().requires_grad_(True)
    zz, rnet = elbo._SisrHR.apply(mu, hr32, z32, EPS2)
    (dmu,) = torch.autograd.grad([zz, rnet], [mu], [gzz.cuda(), gs.cuda()])
    want_zz = t["mu"].detach() + math.sqrt(EPS2) * draws[2]
    bar_zz = EPS * (t["mu"].detach().abs() + math.sqrt(EPS2) * draws[2].abs())
    assert bool(((zz.detach().cpu().double() - want_zz).abs() <= bar_zz).all())
    assert abs(float(rnet.detach()) - float(ref["out"]["kl_rnet"])) <= ref["bars"]["kl_rnet"]
    first = 0.7 * (t["mu"].detach() - t["im_hr"]) / (EPS2 * t["mu"].numel())
    want, bar = first + gzz.double(), U * (first.abs() + gzz.double().abs())
    ratio = worst_ratio(dmu, want, bar)
    print(f"dmu: worst element at {ratio * 8:.2f} units of 2^-23 * sum|addends| (bar 8)")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", STAGE_CASES)
def test_lr_pass_gradients(case):
    elbo = _elbo()
    ref = reference(case)
    t = ref["t"]
    y32 = ref["out"]["y"].float()                                       # a given y: the reference's, rounded to fp32
    g_lh, g_ks = 0.7, 1.3
    y64, sig64 = y32.double().requires_grad_(True), t["sigma_est"].detach().clone().requires_grad_(True)
    lh, ks = lr_terms(y64, t["im_lr"], sig64, t["sigma_prior"], t["alpha0"])
    want_dy, want_ds = torch.autograd.grad(g_lh * lh + g_ks * ks, [y64, sig64])
    with torch.no_grad():
        a0 = t["alpha0"]
        a = a0 - 1
        beta, beta0 = t["sigma_est"].detach() * a0, t["sigma_prior"] * a0
        x = t["im_lr"]
        m = float(x.numel())
        mk = float(torch.broadcast_shapes(beta.shape, beta0.shape).numel())
        bar_dy = U * (g_lh * (a / beta) * (y32.double() - x).abs() / m)
        t_lh = (g_lh * ((0.5 / beta).abs() + 0.5 * a * (x - y32.double()) ** 2 / beta ** 2) / m).expand(x.shape)
        t_ki = (g_ks * ((a / beta).abs() + (a * beta0 / beta ** 2).abs()) / mk).expand(torch.broadcast_shapes(beta.shape, beta0.shape))
        bar_ds = U * a0 * (t_lh.sum_to_size(beta.shape) + t_ki.sum_to_size(beta.shape))
        a_lh = float((0.5 * beta.log().abs() + 0.5 * torch.digamma(a).abs() + 0.5 * (a / beta) * (x - y32.double()) ** 2).mean()) + 0.5 * math.log(2 * math.pi)
    y = y32.cuda().requires_grad_(True)
    sig = t["sigma_est"].detach().float().cuda().requires_grad_(True)
    sc = elbo._scalars(t["alpha0"].float().cuda(), y.device)
    got_lh, got_ks = elbo._SisrLR.apply(y, sig, t["im_lr"].float().cuda(), t["sigma_prior"].float().cuda(), sc)
    dy, ds = torch.autograd.grad([got_lh, got_ks], [y, sig], [torch.tensor(g_lh).cuda(), torch.tensor(g_ks).cuda()])
    assert abs(float(got_lh.detach()) - float(lh.detach())) <= U * a_lh and abs(float(got_ks.detach()) - float(ks.detach())) <= ref["bars"]["kl_snet"]
    assert ds.shape == sig.shape and dy.shape == y.shape
    for name, got, want, bar in (("dy", dy, want_dy, bar_dy), ("dsigma", ds, want_ds, bar_ds)):
        ratio = worst_ratio(got, want, bar)
        print(f"{name}: worst element at {ratio * 8:.2f} units of 2^-23 * sum|addends| (bar 8)")
        assert ratio <= 1.0, name


def head_reference(t, draws, k, sf, shift, gk, g_knet):
    """float64: kernel, the KL terms and dkinfo for the upstream (gk, g_knet), with the bar U * sum |addends| of dkinfo's closed form:
    sum_j |dq_j| |dq_j / dkinfo_i| over the taps (dq = K (gK - sum gK K), the Jacobian of q by autograd) plus the KL gradients' terms"""
    est = t["kinfo_est"].detach().double().clone().requires_grad_(True)
    gt, kap = t["kinfo_gt"].double(), t["kappa0"].double()
    gamma, rho_eps = draws[0].double(), draws[1].double()
    cov, rho_raw, _ = covariance(est, kap, t["r2"], gamma, rho_eps)
    kernel = loss.sigma2kernel(cov, k, sf, shift)
    knet, k0, k1, k2 = knet_terms(est, gt, kap, t["r2"], t["penalty_K"])
    (want,) = torch.autograd.grad((gk * kernel).sum() + g_knet * knet, est)

    def q_of(e):
        c, _, _ = covariance(e, kap, t["r2"], gamma, rho_eps)
        centre = k // 2 + (0.5 * (sf - k % 2) if shift else 0)
        grid = torch.arange(k, dtype=torch.float64) - centre
        z = torch.stack(torch.meshgrid(grid, grid, indexing="ij"), dim=2).view(1, -1, 2, 1)
        return -0.5 * z.transpose(2, 3).matmul(torch.inverse(c)).matmul(z).squeeze(-1).squeeze(-1)
    n = est.shape[0]
    jac = torch.autograd.functional.jacobian(q_of, est.detach())                      # [N, k^2, N, 3]
    jac = torch.stack([jac[i, :, i, :] for i in range(n)])                            # [N, k^2, 3]
    with torch.no_grad():
        kf, gf = kernel.view(n, -1), gk.view(n, -1)
        dq = kf * (gf - (gf * kf).sum(1, keepdim=True))
        addends = (dq.abs().unsqueeze(2) * jac.abs()).sum(1)
        ak, e, w = kap - 1, est.detach(), abs(g_knet) * t["penalty_K"][1] / 3 / n
        addends[:, :2] += w * ak * (1 / e[:, :2] + gt[:, :2] / e[:, :2] ** 2)
        addends[:, 2] += w * t["penalty_K"][0] * (e[:, 2] - gt[:, 2]).abs() / t["r2"]
    return kernel.detach(), (knet.detach(), k0.detach(), k1.detach(), k2.detach()), want, U * addends, rho_raw.detach()


def run_head(t, draws, k, sf, shift, gk, g_knet):
    elbo = _elbo()
    est = t["kinfo_est"].detach().float().cuda().requires_grad_(True)
    outs = elbo._SisrHead.apply(est, t["kinfo_gt"].float().cuda(), draws[0].float().cuda(), draws[1].float().cuda(), t["kappa0"].float().cuda(),
                                float(t["r2"]), float(t["penalty_K"][0]), float(t["penalty_K"][1]), k, sf, shift)
    (dk,) = torch.autograd.grad([outs[0], outs[1]], [est], [gk.float().cuda(), torch.tensor(float(g_knet)).cuda()])
    return outs, dk


# the golden's k; the training k and sf; an even k with shift=True (k 8, sf 2: the centre moves to 5); odd k with shift
@pytest.mark.parametrize("n,k,sf,shift", [(2, 9, 2, False), (2, 21, 4, False), (2, 8, 2, True), (1, 5, 3, True), (3, 25, 4, False)])
def test_head_kernel_terms_and_gradient(n, k, sf, shift):
    t, draws = make_inputs((n, 1, 12, 12, 5, "Direct", "ss"), seed=40 + k)
    t, draws = to(t, draws, dtype=torch.float64)
    gk = torch.randn(n, 1, k, k, generator=torch.Generator().manual_seed(k), dtype=torch.float64)
    kernel, terms, want, bar, rho_raw = head_reference(t, draws, k, sf, shift, gk, 1.3)
    assert float(rho_raw.abs().max()) < 1.0
    outs, dk = run_head(t, draws, k, sf, shift, gk, 1.3)
    ratio = (outs[0].cpu().double() - kernel).abs() / (EPS * kernel + 1e-37)
    assert float(ratio.max()) <= 1.0
    for got, w_ in zip(outs[1:], terms):
        assert abs(float(got.detach()) - float(w_)) <= U * max(abs(float(w_)), 1e-30) + 1e-12       # (the term-wise bars: test_values_*)
    ratio = worst_ratio(dk, want, bar)
    print(f"dkinfo: worst element at {ratio * 8:.2f} units of 2^-23 * sum|addends| (bar 8)")
    assert ratio <= 1.0


def test_singular_sample_is_nudged_alone():
    """batch of three; the middle sample has v1 = v2 = 4 and a correlation clamped to 1: det = 0 exactly.  Its kernel is that of the
    covariance plus 1e-5 I (float64 loss.sigma2kernel); samples 0 and 2 are bit for bit what they are when run alone"""
    t, draws = make_inputs((3, 1, 12, 12, 5, "Direct", "ss"), seed=77)
    t = dict(t)
    t["kinfo_est"] = t["kinfo_est"].clone()
    t["kinfo_est"][1] = torch.tensor([2.0, 2.0, 0.99])
    gamma, rho_eps = draws[0].clone(), draws[1].clone()
    gamma[1] = 25.0
    rho_eps[1] = 2.0                                                     # 0.99 + 0.01 * 2 >= 1
    draws = (gamma, rho_eps, draws[2])
    k, sf = 9, 2
    gk = torch.randn(3, 1, k, k, generator=torch.Generator().manual_seed(3))
    outs, dk = run_head(t, draws, k, sf, False, gk, 0.0)
    cov, _, _ = covariance(t["kinfo_est"].double(), t["kappa0"].double(), t["r2"], gamma.double(), rho_eps.double())
    assert float(cov[1, 0, 0, 0] * cov[1, 0, 1, 1] - cov[1, 0, 0, 1] ** 2) == 0.0 and float(cov[1, 0, 0, 0]) == 4.0 and float(cov[1, 0, 0, 1]) == 4.0
    want = loss.sigma2kernel(cov[1:2] + 1e-5 * torch.eye(2, dtype=torch.float64).view(1, 1, 2, 2), k, sf, False)
    got = outs[0][1:2].cpu().double()
    assert bool(torch.isfinite(got).all()) and bool(((got - want).abs() <= EPS * want + 1e-37).all())
    assert bool(torch.isfinite(dk).all())
    for i in (0, 2):
        ti = {key: (v[i:i + 1] if isinstance(v, torch.Tensor) and v.dim() == 2 else v) for key, v in t.items()}
        oi, dki = run_head(ti, tuple(d[i:i + 1] for d in draws), k, sf, False, gk[i:i + 1], 0.0)
        assert torch.equal(oi[0][0], outs[0][i]) and torch.equal(dki[0], dk[i])


# ---- the whole objective's gradients, through the degradation ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES[:8])
def test_composite_gradients_against_float64_and_the_parent_route(case):
    """dmu, dsigma, dkinfo of the whole objective: each route's error against float64 as max-abs over the tensor divided by the reference's
    largest entry; the device route's is at most 4x the parent route's (the fp32 torch composition on the device, same draws) and the
    device route stays inside the bars of test_elbo_sisr_hip_against_torch_on_the_device"""
    ref = reference(case)
    _, _, hip = run_hip(case)
    _, _, _, parent = run_composition(case, "cuda", torch.float32)
    for name in GRAD_KEYS:
        want = ref["grads"][name]
        e_hip, e_par = rel_err(hip[name], want), rel_err(parent[name], want)
        print(f"{case} d{name}: device route {e_hip:.3e}, parent route {e_par:.3e} (ratio {e_hip / max(e_par, 1e-300):.2f})")
    for name in GRAD_KEYS:
        want = ref["grads"][name]
        assert rel_err(hip[name], want) <= 4 * rel_err(parent[name], want), name
    want = ref["grads"]
    got_mu = hip["mu"].cpu().double()
    assert float(got_mu.sum()) == pytest.approx(float(want["mu"].sum()), rel=1e-4) and float(got_mu.abs().max()) == pytest.approx(float(want["mu"].abs().max()), rel=1e-4)
    # dsigma: rel 1e-4 in the error measure above for every layout; element by element, as the existing test compares its [N,1,1,1]
    # sigma_est, for that layout.  (An element of a per-pixel sigma_est is the difference of two terms, 0.5 n / beta and
    # 0.5 (alpha0 - 1) sum (x - y)^2 / beta^2, that cancel to 1e-4 of themselves at some pixels: there the fp32 rounding of y alone, which
    # both routes share, exceeds 1e-4 of the element.)
    assert rel_err(hip["sigma_est"], want["sigma_est"]) <= 1e-4
    if case[6][0] == "s":
        assert hip["sigma_est"].cpu().double().reshape(-1).tolist() == pytest.approx(want["sigma_est"].reshape(-1).tolist(), rel=1e-4)
    assert hip["kinfo_est"].cpu().double().reshape(-1).tolist() == pytest.approx(want["kinfo_est"].reshape(-1).tolist(), rel=2e-3, abs=1e-4)


@pytest.mark.parametrize("down", ["Bicubic", "Direct"])
def test_same_seed_two_routes(down):
    """draws=None: the same seed gives the draws of the torch route (order and primitives), on the golden's inputs"""
    G = json.load(open(os.path.join(GOLDEN, "loss_sisr.json")))

    def run(impl):
        t = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in golden_inputs(G).items()}
        for k in GRAD_KEYS:
            t[k].requires_grad_(True)
        torch.manual_seed(G["torch_seed"])
        out, det = loss.elbo_sisr(downsampler=down, impl=impl, **t)
        state = torch.cuda.get_rng_state()
        out.backward()
        return ([float(out)] + [float(v) for v in det[:7]], float(t["mu"].grad.double().sum()), float(t["mu"].grad.abs().max()),
                [float(v) for v in t["sigma_est"].grad.reshape(-1)], [float(v) for v in t["kinfo_est"].grad.reshape(-1)], det[7], state)
    want, got = run("torch"), run("hip")
    print(down, "torch", want[:5], "\nhip", got[:5])
    assert got[0] == pytest.approx(want[0], rel=2e-5)
    assert got[1] == pytest.approx(want[1], rel=1e-4) and got[2] == pytest.approx(want[2], rel=1e-4)
    assert got[3] == pytest.approx(want[3], rel=1e-4)
    assert got[4] == pytest.approx(want[4], rel=2e-3, abs=1e-4)
    assert float((got[5] - want[5]).abs().max()) <= 1e-5 * float(want[5].max())
    assert torch.equal(got[6], want[6])                                  # the generator advanced identically


def test_batch_independence_and_reproducibility():
    """two runs are bitwise equal; each sample's kernel, dmu and dkinfo are bitwise those of the sample in a batch of one after the exact
    rescale by the means' 1/N (N = 2: a power of two)"""
    case = CASES[0]
    a, b = run_hip(case), run_hip(case)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and all(torch.equal(a[2][k], b[2][k]) for k in GRAD_KEYS)
    t, draws = make_inputs(case)
    for i in range(2):
        ti = {k: (v[i:i + 1] if isinstance(v, torch.Tensor) and v.dim() > 1 else v) for k, v in t.items()}
        ti, di = to(ti, tuple(d[i:i + 1] for d in draws), device="cuda")
        for k in GRAD_KEYS:
            ti[k] = ti[k].clone().requires_grad_(True)
        total, parts = _elbo().elbo_sisr(downsampler=case[5], draws=di, **ti)
        total.backward()
        assert torch.equal(parts[7][0], a[1][7][i])
        assert torch.equal(ti["mu"].grad[0], 2.0 * a[2]["mu"][i]) and torch.equal(ti["kinfo_est"].grad[0], 2.0 * a[2]["kinfo_est"][i])


def test_no_host_synchronisation():
    """after a warm-up, value + backward enqueue without the host ever waiting for the device (torch's sync debug mode raises on any
    synchronising call); the same mode does catch torch.inverse, the one wait of the torch route"""
    case = CASES[1]
    run_hip(case)
    t, _ = to(*make_inputs(case), device="cuda")
    for k in GRAD_KEYS:
        t[k] = t[k].clone().requires_grad_(True)
    cov = torch.eye(2, device="cuda").repeat(2, 1, 1, 1) * 2.0
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, parts = _elbo().elbo_sisr(downsampler="Direct", degrade_impl="hip", **t)      # generator draws
        total.backward()
        caught = False
        try:
            torch.inverse(cov)
        except RuntimeError:
            caught = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total)) and all(t[k].grad is not None for k in GRAD_KEYS)
    if not caught:
        pytest.skip("torch.inverse does not raise under set_sync_debug_mode('error') on this build: the mode proves nothing here")


def test_value_and_backward_replay_from_a_graph():
    """after a warm-up, value + backward captured on one stream with explicit draws; replayed on two different inputs, bitwise equal to eager"""
    case = CASES[1]
    elbo = _elbo()
    sets = [to(*make_inputs(case, seed=s), device="cuda") for s in (21, 22)]
    tensor_keys = [k for k, v in sets[0][0].items() if isinstance(v, torch.Tensor)]

    def call(t, draws):
        total, parts = elbo.elbo_sisr(downsampler=case[5], degrade_impl="hip", draws=draws, **t)
        return [total.detach()] + list(parts) + list(torch.autograd.grad(total, [t[k] for k in GRAD_KEYS]))

    def eager(t, draws):
        t = dict(t)
        for k in GRAD_KEYS:
            t[k] = t[k].clone().requires_grad_(True)
        return [o.clone() for o in call(t, draws)]
    want = [eager(*s) for s in sets]                                     # (also the warm-up of this shape)
    static = {k: (torch.zeros_like(v) if k in tensor_keys else v) for k, v in sets[0][0].items()}
    sdraws = tuple(torch.zeros_like(d) for d in sets[0][1])
    for k in GRAD_KEYS:
        static[k].requires_grad_(True)

    def load(t, draws):
        with torch.no_grad():
            for k in tensor_keys:
                static[k].copy_(t[k])
            for d, s in zip(sdraws, draws):
                d.copy_(s)
    load(*sets[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(static, sdraws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = call(static, sdraws)
    for s, w in zip(sets, want):
        load(*s)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, w))


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------
def test_upstream_gradient_parts_and_double_backward():
    case = CASES[1]
    total, parts, g1 = run_hip(case)
    _, _, g4 = run_hip(case, scale=4.0)
    assert all(torch.equal(g4[k], 4.0 * g1[k]) for k in GRAD_KEYS)       # the upstream scalar enters as one factor: a power of two is exact
    _, _, g3 = run_hip(case, scale=3.0)
    ref = reference(case)
    for k, bar in zip(GRAD_KEYS, (1e-4, 1e-4, 2e-3)):                    # 3.0: within the composite bars
        assert rel_err(g3[k], 3.0 * ref["grads"][k]) <= bar, k
    assert total.requires_grad and not any(p.requires_grad for p in parts)
    t, draws = to(*make_inputs(case), device="cuda")
    mu = t["mu"].clone().requires_grad_(True)
    total, _ = _elbo().elbo_sisr(downsampler=case[5], draws=draws, **dict(t, mu=mu))
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(total, mu, create_graph=True)


def test_strided_inputs_go_through_contiguous():
    """a channels-last ``mu`` and a transposed ``kinfo_est`` give the bits of the dense ones"""
    case = CASES[1]
    dense = run_hip(case)

    def mutate(t):
        t["mu"] = t["mu"].contiguous(memory_format=torch.channels_last)
        t["kinfo_est"] = t["kinfo_est"].t().contiguous().t()
        assert not t["kinfo_est"].is_contiguous()
    strided = run_hip(case, mutate=mutate)
    assert torch.equal(strided[0], dense[0]) and all(torch.equal(strided[2][k], dense[2][k]) for k in GRAD_KEYS)


def test_float_alpha0_and_kappa0_are_held_to_the_same_bars():
    """Python floats: alpha0's digamma is taken on the host (it may differ from the device's in the last bit: only ``lh`` sees it)"""
    case = CASES[0]
    total, parts, grads = run_hip(case, floats=True)
    check_values(total, parts, reference(case))
    a = run_hip(case)
    assert all(torch.equal(x, y) for x, y in zip(parts[1:], a[1][1:])) and all(torch.equal(grads[k], a[2][k]) for k in GRAD_KEYS)


def test_loss_keyword_forwards_to_the_device_path():
    case = CASES[1]
    t, _ = to(*make_inputs(case), device="cuda")
    torch.manual_seed(5)
    got = loss.elbo_sisr(downsampler="Direct", impl="hip", degrade_impl="hip", **t)
    torch.manual_seed(5)
    want = _elbo().elbo_sisr(downsampler="Direct", degrade_impl="hip", **t)
    assert torch.equal(got[0], want[0]) and all(torch.equal(x, y) for x, y in zip(got[1], want[1]))
    torch.manual_seed(5)
    via_torch = loss.elbo_sisr(downsampler="Direct", impl="hip", **t)       # degrade_impl defaults to "torch" there and is forwarded
    assert float(via_torch[0]) == pytest.approx(float(want[0]), rel=2e-5)


# ---- inside the training loop ---------------------------------------------------------------------------------------------------------------
def test_sisr_training_loop_with_the_device_objective():
    """the loop of tests/test_sisr_train_gpu.py::test_sisr_training_loop_shape with impl="hip": the loss goes down; the first step's loss and
    per-sub-network gradient norms agree with impl="torch" from the same seed within that file's 1e-4"""
    from test_sisr_train_gpu import SMALL, build
    from virnet_amd.utils.synth import synth_images
    sf, n = 2, 2
    im_lr = synth_images(n, 3, 16, 16).cuda()
    im_hr = synth_images(n, 3, 32, 32, seed=3).cuda()
    kinfo_gt = torch.tensor([[1.2, 0.8, 0.1], [2.0, 1.5, -0.3]], device="cuda")
    nlevel = torch.empty((n, 1, 1, 1), device="cuda").fill_(2e-3)
    alpha0 = 0.5 * torch.tensor([9.0 ** 2], device="cuda")
    kappa0 = torch.tensor([50.0], device="cuda")
    first = {}
    for impl, steps in (("torch", 1), ("hip", 5)):
        net, _ = build(SMALL, seed=6)
        opt = torch.optim.Adam(net.parameters(), lr=2e-4)
        groups = {key: [p for nm, p in net.named_parameters() if key in nm.lower()] for key in ("rnet", "snet", "knet")}
        torch.manual_seed(0)
        losses = []
        for step in range(steps):
            opt.zero_grad()
            mu, kinfo_est, sigma_est = net(im_lr, sf)
            total, detail = loss.elbo_sisr(mu=mu, sigma_est=sigma_est, kinfo_est=kinfo_est, im_hr=im_hr, im_lr=im_lr, sigma_prior=nlevel, alpha0=alpha0,
                                           kinfo_gt=kinfo_gt, kappa0=kappa0, r2=1e-4, eps2=1e-5, sf=sf, k_size=9, penalty_K=[0.02, 2], shift=False,
                                           downsampler="Bicubic", impl=impl, degrade_impl="hip" if impl == "hip" else "torch")
            total.backward()
            norms = [float(torch.nn.utils.clip_grad_norm_(groups[key], lim)) for key, lim in (("rnet", 5e2), ("snet", 1e2), ("knet", 5e2))]
            if step == 0:
                first[impl] = (float(total.detach()), norms)
            opt.step()
            assert torch.isfinite(total) and detail[7].shape == (n, 1, 9, 9)
            losses.append(float(total.detach()))
    assert losses[-1] < losses[0], losses
    print("first step (loss, [rnet, snet, knet] gradient norms):", first)
    assert first["hip"][0] == pytest.approx(first["torch"][0], rel=1e-4)
    assert first["hip"][1] == pytest.approx(first["torch"][1], rel=1e-4)
