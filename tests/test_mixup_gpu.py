"""The device MixUp and the real-noise batch (virnet_amd/datagen.py: mixup, real_batch; csrc/datagen.hip) against their numpy definitions,
which tests/test_mixup_host.py pins to the reference's own ``MixUp_AUG.aug``.  Everything is compared bit for bit: the reference rounds
``1 - lam``, both products and the sum separately, and a kernel that fuses the multiply-add differs on about a fifth of the elements.
Pool, parameters and patch sizes: tests/datagen_cases.py; the mix: tests/mixup_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import datagen_cases as dc
import mixup_cases as mc
from conftest import load_golden
from virnet_amd import _native, datagen, elbo

pytestmark = pytest.mark.gpu
K = 7
ORDER = np.asarray([8, 2, 5, 0, 7, 1, 3, 6, 4])


@pytest.fixture(scope="module")
def pool():
    return datagen.ImagePool.paired(list(dc.images(0)), list(dc.images(1)), "cuda")


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared cases are read-only)


def test_mixup_is_the_reference_on_the_golden_batch():
    G = load_golden("mixup")
    mix = datagen.MixParams(G["perm"], G["lam"])
    out_gt, out_noisy = datagen.mixup(cuda(G["gt"]), cuda(G["noisy"]), mix)
    assert out_gt.shape == out_noisy.shape == (9, 3, 20, 20) and out_gt.dtype == out_noisy.dtype == torch.float32
    assert dc.same_bits(out_gt, G["out_gt"]) and dc.same_bits(out_noisy, G["out_noisy"])
    assert dc.same_bits(out_gt, datagen.mixup_np(G["gt"], mix)) and dc.same_bits(out_noisy, datagen.mixup_np(G["noisy"], mix))


@pytest.mark.parametrize("shape", mc.SHAPES + [(9, 3, 20, 20)], ids=str)
def test_mixup_is_the_definition_bit_for_bit(shape):
    a, b = mc.tensors(shape)
    mix = mc.mix() if shape[0] == 9 else mc.mix_for(shape[0])
    ta, tb = cuda(a), cuda(b)
    out_a, out_b = datagen.mixup(ta, tb, mix)
    assert dc.same_bits(out_a, datagen.mixup_np(a, mix)) and dc.same_bits(out_b, datagen.mixup_np(b, mix))
    assert torch.equal(ta, cuda(a)) and torch.equal(tb, cuda(b))          # the inputs are left alone
    again = datagen.mixup(ta, tb, mix.to("cuda"))
    assert torch.equal(again[0], out_a) and torch.equal(again[1], out_b)


def test_mixup_of_views_that_are_4_byte_aligned_only():
    """per % 4 == 0, but both inputs start one element into a larger buffer: the 4-byte form"""
    shape = (9, 3, 20, 20)
    a, b = mc.tensors(shape)
    count = int(np.prod(shape))
    views = []
    for v in (a, b):
        buf = torch.full((count + 5,), float("nan"), device="cuda")
        buf[1:1 + count] = cuda(v).reshape(-1)
        views.append(buf[1:1 + count].view(shape))
    assert all(v.is_contiguous() and v.data_ptr() % 16 == 4 for v in views)
    out_a, out_b = datagen.mixup(views[0], views[1], mc.mix())
    assert dc.same_bits(out_a, datagen.mixup_np(a, mc.mix())) and dc.same_bits(out_b, datagen.mixup_np(b, mc.mix()))


@pytest.mark.parametrize("p", dc.PATCHES)
def test_real_batch_is_the_definition_bit_for_bit(pool, p):
    want_noisy, want_gt = mc.expected(p)
    im_noisy, im_gt, sigma_gt = datagen.real_batch(pool, dc.params(p), p, mc.mix(), k_size=None)
    assert sigma_gt is None and im_noisy.shape == im_gt.shape == (dc.N, 3, p, p) and im_noisy.dtype == im_gt.dtype == torch.float32
    assert dc.same_bits(im_noisy, want_noisy) and dc.same_bits(im_gt, want_gt)
    pair = datagen.pair_batch(pool, dc.params(p), p)
    mixed_gt, mixed_noisy = datagen.mixup(*pair[::-1], mc.mix())
    assert torch.equal(im_noisy, mixed_noisy) and torch.equal(im_gt, mixed_gt)
    # lam = 1 (sample 2): the sample's own pair_batch rows; lam = 0 (sample 1): its partner's
    assert mc.LAM[2] == 1.0 and mc.LAM[1] == 0.0
    for got, rows in ((im_noisy, pair[0]), (im_gt, pair[1])):
        assert torch.equal(got[2], rows[2]) and torch.equal(got[1], rows[mc.PERM[1]])
    again = datagen.real_batch(pool, dc.params(p), p, mc.mix(), k_size=None)
    assert torch.equal(again[0], im_noisy) and torch.equal(again[1], im_gt)          # two identical calls are bitwise equal


def window_float64(noisy: np.ndarray, gt: np.ndarray, k: int) -> torch.Tensor:
    """the Gaussian-window mean of the squared error in float64 (formed in float64 from the fp32 images), reflect border"""
    g1 = elbo.gaussian_taps(k)
    k2 = torch.from_numpy(g1[:, None] * g1[None, :])
    k2 = k2 / k2.sum()
    err2 = torch.from_numpy(noisy.astype(np.float64) - gt.astype(np.float64)) ** 2
    c = err2.shape[1]
    return F.conv2d(F.pad(err2, (k // 2,) * 4, mode="reflect"), k2.expand(c, 1, k, k).contiguous(), groups=c)


@pytest.mark.parametrize("p", dc.PATCHES)
def test_sigma_gt_is_the_variance_prior_of_the_mixed_batch(pool, p):
    floor = 1e-10
    im_noisy, im_gt, sigma_gt = datagen.real_batch(pool, dc.params(p), p, mc.mix(), K, floor)
    assert sigma_gt.shape == (dc.N, 3, p, p) and sigma_gt.dtype == torch.float32
    assert torch.equal(sigma_gt, elbo.noise_estimate(im_noisy, im_gt, K, floor))
    want = window_float64(*mc.expected(p), K)          # the yardstick: fp64 on the numpy definition's images, not on the device's own
    ratio = (sigma_gt.cpu().double() - want.clamp_min(floor)).abs() / (K * K * 2.0 ** -23 * want + floor)
    print(f"P={p}: worst sigma_gt element at {float(ratio.max()):.3f} of its bar")
    assert float(ratio.max()) <= 1.0
    assert torch.equal(datagen.real_batch(pool, dc.params(p), p, mc.mix(), K, floor)[2], sigma_gt)


def _reordered(params, mix, order):
    """the same samples in another order: new sample j is old sample order[j], so its partner's new index is inv[perm[order[j]]]"""
    inv = np.empty_like(order)
    inv[order] = np.arange(order.shape[0])
    return params.select(order), datagen.MixParams(inv[mix.perm[order]], mix.lam[order])


@pytest.mark.parametrize("p", dc.PATCHES)
def test_a_row_does_not_depend_on_its_place_in_the_batch(pool, p):
    base = datagen.real_batch(pool, dc.params(p), p, mc.mix(), K)
    params, mix = _reordered(dc.params(p), mc.mix(), ORDER)
    got = datagen.real_batch(pool, params, p, mix, K)
    assert all(torch.equal(g, b[ORDER]) for g, b in zip(got, base))
    a, b = (cuda(v) for v in mc.tensors((dc.N, 3, p, p)))
    plain = datagen.mixup(a, b, mc.mix())
    moved = datagen.mixup(a[ORDER], b[ORDER], mix)
    assert all(torch.equal(g, w[ORDER]) for g, w in zip(moved, plain))


def _capture(monkeypatch, fn):
    """fn() captured into a graph -> (graph, its results, the stream handle of every launch, the capturing stream)"""
    streams = []
    real = _native.stream_handle
    monkeypatch.setattr(_native, "stream_handle", lambda: (streams.append(real()), streams[-1])[1])
    graph = torch.cuda.CUDAGraph()
    with _native.capture_lock, torch.cuda.graph(graph):
        capture_stream = torch.cuda.current_stream().cuda_stream
        got = fn()
    monkeypatch.undo()
    return graph, got, streams, capture_stream


def test_captured_graphs_follow_the_parameter_and_mix_buffers(pool, monkeypatch):
    p = 33
    first, second = dc.params(p), dc.params(p).select(np.asarray([4, 3, 8, 0, 1, 7, 6, 2, 5]))
    dp, dm = first.to("cuda"), mc.mix().to("cuda")
    a, b = (cuda(v) for v in mc.tensors((dc.N, 3, p, p)))
    want_first = datagen.real_batch(pool, dp, p, dm, K) + datagen.mixup(a, b, dm)          # (also the warm-up: the window's taps are uploaded)
    want_second = datagen.real_batch(pool, second, p, mc.mix(True), K) + datagen.mixup(a, b, mc.mix(True))
    torch.cuda.synchronize()
    graph_r, got_r, streams, capture_stream = _capture(monkeypatch, lambda: datagen.real_batch(pool, dp, p, dm, K))
    assert streams == [capture_stream] * 2                # two launches, both on the capturing stream
    graph_m, got_m, streams, capture_stream = _capture(monkeypatch, lambda: datagen.mixup(a, b, dm))
    assert streams == [capture_stream]                    # one launch
    got = got_r + got_m
    graph_r.replay()
    graph_m.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want_first))
    dp.update(second)                                     # the buffers' contents change, their addresses do not
    dm.update(mc.mix(True))
    graph_r.replay()
    graph_m.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want_second))
    assert not torch.equal(got[0], want_first[0]) and not torch.equal(got[3], want_first[3])
    assert dc.same_bits(got[0], datagen.real_batch_np(list(dc.images(0)), list(dc.images(1)), second, mc.mix(True))[0])


def test_neither_call_synchronises(pool):
    p = 20
    dp, dm = dc.params(p).to("cuda"), mc.mix().to("cuda")
    a, b = (cuda(v) for v in mc.tensors((dc.N, 3, p, p)))
    want = datagen.real_batch(pool, dp, p, dm, K) + datagen.mixup(a, b, dm)          # (the warm-up)
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = datagen.real_batch(pool, dp, p, dm, K) + datagen.mixup(a, b, dm)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_the_batch_feeds_the_objective():
    """train_denoising_real.py:164-171 at N = 2, P = 20: beta0 = alpha0 * sigma_gt as [N,3,P,P] is what elbo.elbo_denoising takes"""
    n, p = 2, 20
    ims, other = list(dc.images(0)), list(dc.images(1))
    small = datagen.ImagePool.paired(ims, other, "cuda")
    params = dc.params(p).select(slice(0, n))
    im_noisy, im_gt, sigma_gt = datagen.real_batch(small, params, p, datagen.MixParams([1, 0], [0.7851624, 0.06652636]), K)
    alpha0 = 0.5 * torch.tensor([float(K * K)], device="cuda")
    beta0 = alpha0 * sigma_gt
    assert beta0.shape == (n, 3, p, p)
    mu = (0.5 * (im_noisy + im_gt)).requires_grad_(True)
    sigma = torch.full((n, 1, p, p), 0.05, device="cuda").requires_grad_(True)
    loss, lh, kl_gauss, kl_igamma = elbo.elbo_denoising(mu, sigma, im_noisy, im_gt, 1e-6, alpha0, beta0)
    loss.backward()
    assert all(bool(torch.isfinite(v)) for v in (loss, lh, kl_gauss, kl_igamma))
    assert bool(torch.isfinite(mu.grad).all()) and bool(torch.isfinite(sigma.grad).all())
