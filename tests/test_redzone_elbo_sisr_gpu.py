"""Red-zone runs of the device SISR objective's launch families (csrc/elbo_sisr.hip): head forward / backward, HR value / gradient,
LR value / gradient and the finishing launches, each inside ``redzone.guarded()`` at a scalar-path shape and at a 16-byte shape.  A green
run means no zone was touched, every output element was written, and the result is bitwise the unguarded one (tests/redzone.py)."""
import pytest
import torch

import redzone
from redzone import guarded
from virnet_amd import elbo

pytestmark = pytest.mark.gpu

ALPHA0, KAPPA0, R2, EPS2 = 40.5, 50.0, 1e-4, 1e-5
# (N, HR h, HR w, sf): HR plane 15 x 21 = 315 and LR plane 5 x 7 = 35 (no multiples of four: scalar accesses); 32 x 24 and 16 x 12 (16-byte)
SHAPES = {"scalar": (1, 15, 21, 3), "vector": (2, 32, 24, 2)}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def run_guarded(call, tensors):
    """``call(**tensors)`` outside the guard, then inside it on ``guard_input`` copies: zones intact, results at home in arenas, every
    element written, no NaN, and guarded == unguarded bit for bit"""
    plain = redzone._flatten(call(**{k: v.clone() for k, v in tensors.items()}))
    torch.cuda.synchronize()
    with guarded() as g:
        got = redzone._flatten(call(**{k: g.input(v) for k, v in tensors.items()}))
        assert got, "the case returned no tensor"
        g.check(got)
        assert all(g.home(t) is not None for t in got)
        got = [t.clone() for t in got]
    assert len(got) == len(plain)
    for i, (a, b) in enumerate(zip(got, plain)):
        assert same_bits(a, b), (i, float((a.double() - b.double()).abs().max()))


def rnd(*shape, seed=0, lo=0.0, hi=1.0):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo).cuda()


@pytest.mark.parametrize("n,k,sf,shift", [(1, 9, 3, False), (2, 21, 4, False), (2, 8, 2, True)])
def test_head_forward_finish_and_backward(n, k, sf, shift):
    est = torch.cat([rnd(n, 2, seed=1, lo=0.5, hi=3.5), rnd(n, 1, seed=2, lo=-0.6, hi=0.6)], 1)
    gt = torch.cat([rnd(n, 2, seed=3, lo=0.5, hi=3.5), rnd(n, 1, seed=4, lo=-0.6, hi=0.6)], 1)
    gamma, rho_eps = rnd(n, 2, seed=5, lo=40.0, hi=60.0), rnd(n, 1, seed=6, lo=-1.0, hi=1.0)
    gk, gs = rnd(n, 1, k, k, seed=7, lo=-1.0, hi=1.0), torch.tensor(1.3).cuda()
    ksc = torch.tensor([KAPPA0]).cuda()

    def call(est, gt, gamma, rho_eps, ksc, gk, gs):
        est = est.detach().requires_grad_(True)
        outs = elbo._SisrHead.apply(est, gt, gamma, rho_eps, ksc, R2, 0.02, 2.0, k, sf, shift)
        (dk,) = torch.autograd.grad([outs[0], outs[1]], [est], [gk, gs])
        return [o.detach() for o in outs[:2]] + [dk]          # (kl_k0..2 are views of kl_knet's four floats)
    run_guarded(call, dict(est=est, gt=gt, gamma=gamma, rho_eps=rho_eps, ksc=ksc, gk=gk, gs=gs))


@pytest.mark.parametrize("name", list(SHAPES))
def test_hr_value_finish_and_gradient(name):
    n, h, w, _ = SHAPES[name]
    mu, hr = rnd(n, 3, h, w, seed=1), rnd(n, 3, h, w, seed=2)
    z, gzz = rnd(n, 3, h, w, seed=3, lo=-2.0, hi=2.0), rnd(n, 3, h, w, seed=4, lo=-1e-3, hi=1e-3)
    gs = torch.tensor(0.7).cuda()

    def call(mu, hr, z, gzz, gs):
        mu = mu.detach().requires_grad_(True)
        zz, rnet = elbo._SisrHR.apply(mu, hr, z, EPS2)
        (dmu,) = torch.autograd.grad([zz, rnet], [mu], [gzz, gs])
        return zz.detach(), rnet.detach(), dmu
    run_guarded(call, dict(mu=mu, hr=hr, z=z, gzz=gzz, gs=gs))


@pytest.mark.parametrize("layout", ["ss", "ps", "cp", "sc"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_lr_value_finish_and_gradient(name, layout):
    n, h, w, sf = SHAPES[name]
    hl, wl = h // sf, w // sf
    shapes = {"s": (n, 1, 1, 1), "p": (n, 1, hl, wl), "c": (n, 3, hl, wl)}
    y, x = rnd(n, 3, hl, wl, seed=1), rnd(n, 3, hl, wl, seed=2)
    sig, pri = rnd(*shapes[layout[0]], seed=3, lo=1e-4, hi=1e-2), rnd(*shapes[layout[1]], seed=4, lo=1e-4, hi=1e-2)
    a0 = torch.tensor([ALPHA0]).cuda()
    g1, g2 = torch.tensor(0.7).cuda(), torch.tensor(1.3).cuda()

    def call(y, x, sig, pri, a0, g1, g2):
        y, sig = y.detach().requires_grad_(True), sig.detach().requires_grad_(True)
        sc = elbo._scalars(a0, y.device)
        lh, ks = elbo._SisrLR.apply(y, sig, x, pri, sc)
        dy, ds = torch.autograd.grad([lh, ks], [y, sig], [g1, g2])
        return lh.detach(), dy, ds
    run_guarded(call, dict(y=y, x=x, sig=sig, pri=pri, a0=a0, g1=g1, g2=g2))


def test_finishing_sum():
    vals = {k: torch.tensor(v).cuda() for k, v in dict(a=1.25, b=2.5, c=-0.75, d=10.0).items()}
    run_guarded(lambda a, b, c, d: elbo._SisrSum.apply(a, b, c, d), vals)


@pytest.mark.parametrize("down", ["Direct", "Bicubic"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_whole_objective(name, down):
    """every launch of value + backward as the product calls them, explicit draws, the device degradation in between"""
    n, h, w, sf = SHAPES[name]
    hl, wl = -(-h // sf), -(-w // sf)
    t = dict(mu=rnd(n, 3, h, w, seed=1), sigma_est=rnd(n, 1, 1, 1, seed=2, lo=1e-4, hi=1e-2),
             kinfo_est=torch.cat([rnd(n, 2, seed=3, lo=0.5, hi=3.5), rnd(n, 1, seed=4, lo=-0.6, hi=0.6)], 1), im_hr=rnd(n, 3, h, w, seed=5),
             im_lr=rnd(n, 3, hl, wl, seed=6), sigma_prior=rnd(n, 1, 1, 1, seed=7, lo=1e-4, hi=1e-2),
             kinfo_gt=torch.cat([rnd(n, 2, seed=8, lo=0.5, hi=3.5), rnd(n, 1, seed=9, lo=-0.6, hi=0.6)], 1), alpha0=torch.tensor([ALPHA0]).cuda(),
             kappa0=torch.tensor([KAPPA0]).cuda(), gamma=rnd(n, 2, seed=10, lo=40.0, hi=60.0), rho_eps=rnd(n, 1, seed=11, lo=-1.0, hi=1.0),
             z_eps=rnd(n, 3, h, w, seed=12, lo=-2.0, hi=2.0))
    if down == "Bicubic":
        from virnet_amd import degrade
        degrade.warm_taps(h, w, sf, "cuda")

    def call(gamma, rho_eps, z_eps, **t):
        for k in ("mu", "sigma_est", "kinfo_est"):
            t[k] = t[k].detach().requires_grad_(True)
        total, parts = elbo.elbo_sisr(r2=R2, eps2=EPS2, sf=sf, k_size=9, penalty_K=[0.02, 2.0], shift=False, downsampler=down, degrade_impl="hip",
                                      draws=(gamma, rho_eps, z_eps), **t)
        grads = torch.autograd.grad(total, [t[k] for k in ("mu", "sigma_est", "kinfo_est")])
        return [total.detach(), parts[0], parts[7]] + list(grads)
    run_guarded(call, t)
