"""Red-zone runs (tests/redzone.py) of the device objective and the variance-prior window: every buffer the kernels are given -- inputs, the
device scalars, the partial-sum workspace, the window taps, the results -- sits between NaN-patterned zones.  Nothing may be written outside
a buffer, no zone value may reach a result, and every element of ``dmu``, ``dsigma`` and ``out`` must have been written."""
import pytest
import torch

from redzone import guarded
from test_elbo_gpu import LOOP, make_inputs

pytestmark = pytest.mark.gpu


def _call(elbo, t, n_mu):
    mus = [m.detach().requires_grad_(True) for m in t["mus"]]
    sigma = t["sigma"].detach().requires_grad_(True)
    out = elbo.elbo_denoising(mus if n_mu > 1 else mus[0], sigma, t["noisy"], t["gt"], 1e-6, t["alpha0"], t["beta0"])
    grads = torch.autograd.grad(out[0], mus + [sigma])
    return [o.detach() for o in out], list(grads)


# the odd shapes of tests/test_elbo_gpu.py (scalar accesses, partial waves, all Cs / Cb forms), the 16-byte form, and the grid-stride shape
@pytest.mark.parametrize("shape,n_mu", [((1, 1, 1, 1, 1, 1), 1), ((2, 3, 1, 1, 17, 19), 1), ((2, 3, 3, 3, 17, 19), 1), ((1, 3, 1, 3, 33, 65), 1),
                                        ((4, 3, 3, 1, 64, 64), 1), ((2, 1, 1, 1, 6, 6), 1), (LOOP, 1), ((2, 3, 1, 1, 17, 19), 2)])
def test_elbo_value_and_gradient(shape, n_mu):
    from virnet_amd import elbo
    host = make_inputs(shape, seed=4, n_mu=n_mu)
    dev = {k: ([m.cuda() for m in v] if k == "mus" else v.cuda()) for k, v in host.items()}
    plain_out, plain_grads = _call(elbo, dev, n_mu)
    torch.cuda.synchronize()
    with guarded() as g:
        inside = {k: ([g.input(m) for m in v] if k == "mus" else g.input(v)) for k, v in dev.items()}
        out, grads = _call(elbo, inside, n_mu)
        # (a list's averaged values are formed by torch arithmetic outside the guard's routes: zones and gradients are what is checked there)
        g.check(grads + (out if n_mu == 1 else []))
        # one partial-sum workspace per value launch went through the guard (an unwritten partial would reach `out` as a NaN)
        assert sum(a.dtype == torch.float64 for a in g.arenas) == n_mu
    assert all(torch.equal(a, b) for a, b in zip(out + grads, plain_out + plain_grads))


@pytest.mark.parametrize("shape,k", [((1, 1, 4, 4), 7), ((2, 3, 17, 19), 7), ((1, 2, 37, 150), 7), ((1, 3, 40, 40), 1), ((1, 3, 40, 40), 31),
                                     ((1, 1, 16, 64), 5), ((1, 1, 17, 65), 5)])
def test_noise_estimate(shape, k, monkeypatch):
    from virnet_amd import elbo
    gen = torch.Generator().manual_seed(8)
    gt = torch.rand(shape, generator=gen).cuda()
    noisy = gt + 0.1 * torch.randn(shape, generator=gen).cuda()
    plain = elbo.noise_estimate(noisy, gt, k)
    torch.cuda.synchronize()
    with guarded() as g:
        taps = g.input(torch.from_numpy(elbo.gaussian_taps(k)).cuda())         # the cached window is uploaded with Tensor.to: guard a copy
        monkeypatch.setattr(elbo, "_device_taps", lambda k_size, device: taps)
        out = elbo.noise_estimate(g.input(noisy), g.input(gt), k)
        g.check(out)
    assert torch.equal(out, plain)
