"""The reference of the device SISR objective's tests: ``loss.elbo_sisr`` (loss/ELBO_simple.py:82-138) restated as a composition of
loss.py's own public pieces -- ``kl_gauss``, ``kl_inverse_gamma``, ``sigma2kernel``, ``blur_downsample(impl="torch")`` and the likelihood
expression -- on explicit draws, in whatever dtype and on whatever device its inputs have.  tests/test_elbo_sisr_host.py anchors it to the
reference's golden values (fp32, the generator's draws); tests/test_elbo_sisr_gpu.py evaluates it in float64 on the CPU."""
from math import log, pi, sqrt

import numpy as np
import torch

from virnet_amd import loss

R2, EPS2, KAPPA0, PENALTY_K = 1e-4, 1e-5, 50.0, (0.02, 2.0)
ALPHA0 = 0.5 * 9.0 ** 2


def golden_inputs(G):
    """the seeded inputs of tests/test_loss.py::test_elbo_sisr_matches_reference_golden (fp32, CPU)"""
    g = np.random.Generator(np.random.Philox(key=G["seed"]))
    n, sf, (hl, wl) = G["n"], G["sf"], G["lr_hw"]
    t = {}
    t["mu"] = torch.from_numpy(g.random((n, 3, hl * sf, wl * sf), dtype=np.float32))
    t["sigma_est"] = torch.from_numpy(g.random((n, 1, 1, 1), dtype=np.float32) * 0.01 + 1e-4)
    t["kinfo_est"] = torch.from_numpy(np.stack([g.random(n) * 3 + 0.5, g.random(n) * 3 + 0.5, g.random(n) * 1.2 - 0.6], 1).astype(np.float32))
    t["im_hr"] = torch.from_numpy(g.random((n, 3, hl * sf, wl * sf), dtype=np.float32))
    t["im_lr"] = torch.from_numpy(g.random((n, 3, hl, wl), dtype=np.float32))
    t["sigma_prior"] = torch.from_numpy(g.random((n, 1, 1, 1), dtype=np.float32) * 0.01 + 1e-4)
    t["kinfo_gt"] = torch.from_numpy(np.stack([g.random(n) * 3 + 0.5, g.random(n) * 3 + 0.5, g.random(n) * 1.2 - 0.6], 1).astype(np.float32))
    t["alpha0"] = 0.5 * torch.tensor([G["var_window"] ** 2], dtype=torch.float32)
    t["kappa0"] = torch.tensor([G["kappa0"]])
    t.update(r2=G["r2"], eps2=G["eps2"], sf=sf, k_size=G["k_size"], penalty_K=G["penalty_K"], shift=False)
    return t


def covariance(kinfo_est, kappa0, r2, gamma, rho_eps):
    """(cov [N,1,2,2], rho before the clamp, v [N,2]) of ELBO_simple.py:66-80 on explicit draws: v = kinfo kappa0 / gamma"""
    v = kinfo_est[:, :2] * kappa0 / gamma
    v1, v2 = torch.chunk(v, 2, dim=1)
    rho_raw = kinfo_est[:, 2].unsqueeze(1) + sqrt(r2) * rho_eps
    direction = v1.detach().sqrt() * v2.detach().sqrt() * torch.clamp(rho_raw, min=-1, max=1)
    return torch.cat([v1, direction, direction, v2], dim=1).view(-1, 1, 2, 2), rho_raw, v


def knet_terms(kinfo_est, kinfo_gt, kappa0, r2, penalty_K):
    k0 = loss.kl_inverse_gamma(kappa0 * kinfo_est[:, 0], kappa0 - 1, kappa0 * kinfo_gt[:, 0])
    k1 = loss.kl_inverse_gamma(kappa0 * kinfo_est[:, 1], kappa0 - 1, kappa0 * kinfo_gt[:, 1])
    k2 = loss.kl_gauss(kinfo_est[:, 2], kinfo_gt[:, 2], r2) * penalty_K[0]
    return (k0 + k1 + k2) / 3 * penalty_K[1], k0, k1, k2


def lr_terms(y, im_lr, sigma_est, sigma_prior, alpha0):
    """(lh, kl_snet): the likelihood expression of ELBO_simple.py:55-59 on a given degraded sample, and the inverse-Gamma KL"""
    beta, beta0 = sigma_est * alpha0, sigma_prior * alpha0
    lh = (0.5 * log(2 * pi) + 0.5 * (beta.log() - (alpha0 - 1).digamma()) + 0.5 * (alpha0 - 1).div(beta) * (im_lr - y) ** 2).mean()
    return lh, loss.kl_inverse_gamma(beta, alpha0 - 1, beta0)


def composition(t, draws, downsampler):
    gamma, rho_eps, z_eps = draws
    kl_rnet = loss.kl_gauss(t["mu"], t["im_hr"], t["eps2"])
    kl_knet, k0, k1, k2 = knet_terms(t["kinfo_est"], t["kinfo_gt"], t["kappa0"], t["r2"], t["penalty_K"])
    cov, rho_raw, v = covariance(t["kinfo_est"], t["kappa0"], t["r2"], gamma, rho_eps)
    kernel = loss.sigma2kernel(cov, t["k_size"], t["sf"], t["shift"])
    zz = t["mu"] + z_eps * sqrt(t["eps2"])
    y = loss.blur_downsample(zz, kernel, t["sf"], downsampler, impl="torch")
    lh, kl_snet = lr_terms(y, t["im_lr"], t["sigma_est"], t["sigma_prior"], t["alpha0"])
    total = lh + kl_rnet + kl_snet + kl_knet
    return dict(loss=total, lh=lh, kl_rnet=kl_rnet, kl_snet=kl_snet, kl_knet=kl_knet, kl_k0=k0, kl_k1=k1, kl_k2=k2, kernel=kernel, cov=cov,
                rho_raw=rho_raw, v=v, zz=zz, y=y)
