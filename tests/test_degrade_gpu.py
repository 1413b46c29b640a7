"""The device degradation (virnet_amd/degrade.py, csrc/degrade.hip) against float64 CPU references: forward, both adjoints, the bitwise
properties, the ELBO opt-in, the evaluation input and table, and graph capture.

Reference: the bordered image (index gather, so that autograd sees the fold) -> grouped ``F.conv2d`` -> ``[::sf]`` or the tap-matrix product,
all in float64.  For border "reflect" that is ``loss.blur_downsample`` on float64 CPU tensors (pinned by the reference's golden), for
"symmetric" ``scipy.ndimage.correlate(mode="reflect")``; test_reference_is_the_named_reference holds it to both.

Bars (derived, not tuned):
  forward, gx   |got - ref| <= k^2 * 2^-23 * S, S = the same operator in float64 on |x|, |kernel|, |taps| (for gx: its adjoint on |gy|),
                per element: a few fp32 ulps of sum |w||x|
  gk            within 1e-4 * max|gk| of the sample (the bar tests/test_backward_gpu.py holds weight gradients to)
"""
import glob
import json
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from virnet_amd import _native, degrade, loss, sisr_eval
from virnet_amd import eval as veval

pytestmark = pytest.mark.gpu

SHAPES = {                      # name: (n, c, h, w, k, signed kernel)
    "fold_both_sides": (2, 3, 12, 15, 21, False),       # p = 10: both borders fold onto the same pixels
    "pad_limit": (1, 1, 11, 11, 21, False),             # p = dim - 1
    "ceil_sizes": (2, 3, 44, 52, 21, False),            # not divisible by sf
    "several_tiles": (1, 3, 150, 133, 21, False),       # 16 x 32 output tiles and 8 x 32 gx tiles crossed in both axes, sf = 4 included
    "k5": (3, 3, 40, 40, 5, False),
    "k1": (3, 3, 40, 40, 1, False),
    "signed": (2, 3, 44, 52, 21, True),
}
MODES = [("direct", 1)] + [(d, sf) for d in ("direct", "bicubic") for sf in (2, 3, 4)]


def _fold_index(n, p, border):
    q = np.arange(-p, n + p)
    sym = int(border == "symmetric")
    return torch.from_numpy(np.where(q < 0, -q - sym, np.where(q >= n, 2 * n - 2 + sym - q, q)))


def _taps64(n_in, sf, absolute=False):
    idx, wgt = degrade.tap_table(n_in, sf)
    return torch.from_numpy(degrade.densify(idx, np.abs(wgt) if absolute else wgt, n_in))


def ref_op(x, ker, sf, mode, border, abs_taps=False):
    """float64 CPU, differentiable in x and ker"""
    n, c, h, w = x.shape
    k = ker.shape[-1]
    pad = x.index_select(2, _fold_index(h, k // 2, border)).index_select(3, _fold_index(w, k // 2, border))
    blur = F.conv2d(pad.reshape(1, n * c, h + k - 1, w + k - 1), ker.repeat_interleave(c, 0), groups=n * c).view(n, c, h, w)
    if mode == "direct":
        return blur[:, :, ::sf, ::sf]
    return _taps64(h, sf, abs_taps) @ blur @ _taps64(w, sf, abs_taps).t()


def _inputs(name):
    n, c, h, w, k, signed = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.rand(n, c, h, w, generator=g)
    ker = torch.rand(n, 1, k, k, generator=g)
    if signed:
        ker = ker - 0.5
        ker = ker / ker.abs().sum((2, 3), keepdim=True)
    else:
        ker = ker / ker.sum((2, 3), keepdim=True)
    return x, ker, g


def test_reference_is_the_named_reference():
    from scipy import ndimage
    x, ker, _ = _inputs("ceil_sizes")
    x64, k64 = x.double(), ker.double()
    for mode in ("direct", "bicubic"):
        assert float((ref_op(x64, k64, 3, mode, "reflect") - loss.blur_downsample(x64, k64, 3, mode)).abs().max()) <= 1e-13
    blur = ref_op(x64, k64, 1, "direct", "symmetric")
    want = ndimage.correlate(x64[1, 2].numpy(), k64[1, 0].numpy(), mode="reflect")
    assert np.abs(blur[1, 2].numpy() - want).max() <= 1e-13


@pytest.mark.parametrize("down", ["direct", "bicubic"])
@pytest.mark.parametrize("border", ["reflect", "symmetric"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_adjoints_against_float64(name, border, down):
    x, ker, g = _inputs(name)
    k = ker.shape[-1]
    ulp = k * k * 2.0 ** -23
    for mode, sf in [m for m in MODES if m[0] == down]:
        x64, k64 = x.double().requires_grad_(True), ker.double().requires_grad_(True)
        ref = ref_op(x64, k64, sf, mode, border)
        gy = torch.randn(ref.shape, generator=g)
        gx_ref, gk_ref = torch.autograd.grad(ref, [x64, k64], gy.double())
        xa = x.double().abs().requires_grad_(True)
        s_fwd = ref_op(xa, ker.double().abs(), sf, mode, border, abs_taps=True)
        s_gx, = torch.autograd.grad(s_fwd, xa, gy.double().abs())

        xd, kd = x.cuda().requires_grad_(True), ker.cuda().requires_grad_(True)
        got = degrade.blur_downsample(xd, kd, sf, mode, border=border)
        assert got.shape == ref.shape and got.dtype == torch.float32
        gx, gk = torch.autograd.grad(got, [xd, kd], gy.cuda())
        got, gx, gk = got.detach().cpu().double(), gx.cpu().double(), gk.cpu().double()
        tag = f"{name} {border} {mode} x{sf}"
        e = (got - ref.detach()).abs()
        print(f"{tag}: forward err/bar {float((e / (ulp * s_fwd.detach())).max()):.3f}", end="; ")
        assert bool((e <= ulp * s_fwd.detach()).all()), tag
        e = (gx - gx_ref).abs()
        print(f"gx err/bar {float((e / (ulp * s_gx).clamp_min(1e-300)).max()):.3f}", end="; ")
        assert bool((e <= ulp * s_gx).all()), tag
        assert gk.shape == gk_ref.shape
        for i in range(x.shape[0]):
            bar = 1e-4 * float(gk_ref[i].abs().max())
            err = float((gk[i] - gk_ref[i]).abs().max())
            print(f"gk[{i}] err/bar {err / bar:.3f}", end="; ")
            assert err <= bar, (tag, i, err, bar)
        print()


def test_forward_on_the_loss_tests_inputs():
    """the inputs of tests/test_loss.py::test_blur_downsample_device_path_matches_cpu, its 2e-6 and the derived bar"""
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 64, 48, generator=g)
    ker = torch.rand(2, 1, 21, 21, generator=g)
    ker = ker / ker.sum((2, 3), keepdim=True)
    for mode in ("direct", "bicubic"):
        ref32 = loss.blur_downsample(x, ker, 4, mode)
        ref = ref_op(x.double(), ker.double(), 4, mode, "reflect")
        s = ref_op(x.double().abs(), ker.double().abs(), 4, mode, "reflect", abs_taps=True)
        for got in (degrade.blur_downsample(x.cuda(), ker.cuda(), 4, mode).cpu(), loss.blur_downsample(x.cuda(), ker.cuda(), 4, mode, impl="hip").cpu()):
            assert float((got - ref32).abs().max()) <= 2e-6
            assert bool(((got.double() - ref).abs() <= 441 * 2.0 ** -23 * s).all())


def _run(x, ker, sf, mode, border, gy, need=(True, True)):
    xd, kd = x.detach().requires_grad_(need[0]), ker.detach().requires_grad_(need[1])      # same storage and strides
    y = degrade.blur_downsample(xd, kd, sf, mode, border=border)
    y.backward(gy)
    return y.detach(), xd.grad, kd.grad


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("mode, sf", [("direct", 3), ("bicubic", 4)])
def test_bitwise_properties(mode, sf):
    g = torch.Generator().manual_seed(11)
    x = torch.rand(3, 3, 70, 45, generator=g).cuda()
    ker = torch.rand(3, 1, 21, 21, generator=g).cuda()
    gy = torch.randn(3, 3, -(-70 // sf), -(-45 // sf), generator=g).cuda()
    a, b = _run(x, ker, sf, mode, "reflect", gy), _run(x, ker, sf, mode, "reflect", gy)
    assert all(_same_bits(u, v) for u, v in zip(a, b)), "two runs differ"
    one = _run(x[1:2], ker[1:2], sf, mode, "reflect", gy[1:2])
    assert all(_same_bits(u[1:2], v) for u, v in zip(a, one)), "image 1 of a batch of 3 differs from the same image alone"
    # non-contiguous inputs (a transposed view of the image, a strided slice of the kernel) and an expanded gradient
    xt = x.transpose(2, 3).contiguous().transpose(2, 3)
    kt = torch.stack([ker, ker + 1], -1)[..., 0]
    assert not xt.is_contiguous() and not kt.is_contiguous()
    assert all(_same_bits(u, v) for u, v in zip(a, _run(xt, kt, sf, mode, "reflect", gy)))
    ones = _run(x, ker, sf, mode, "reflect", torch.ones((), device="cuda").expand_as(gy))
    assert all(_same_bits(u, v) for u, v in zip(ones, _run(x, ker, sf, mode, "reflect", torch.ones_like(gy))))


def test_needs_input_grad_is_respected(monkeypatch):
    g = torch.Generator().manual_seed(12)
    x, ker = torch.rand(2, 3, 40, 33, generator=g).cuda(), torch.rand(2, 1, 21, 21, generator=g).cuda()
    gy = torch.randn(2, 3, 20, 17, generator=g).cuda()
    calls = []
    for name in ("_blur_grad_image", "_blur_grad_kernel"):
        monkeypatch.setattr(degrade, name, (lambda f, n: lambda *a, **kw: (calls.append(n), f(*a, **kw))[1])(getattr(degrade, name), name))
    full = _run(x, ker, 2, "bicubic", "reflect", gy)
    assert calls == ["_blur_grad_image", "_blur_grad_kernel"]
    del calls[:]
    only_x = _run(x, ker, 2, "bicubic", "reflect", gy, need=(True, False))
    assert calls == ["_blur_grad_image"] and only_x[2] is None and _same_bits(only_x[1], full[1])      # no gk workspace, no gk launch
    del calls[:]
    only_k = _run(x, ker, 2, "bicubic", "reflect", gy, need=(False, True))
    assert calls == ["_blur_grad_kernel"] and only_k[1] is None and _same_bits(only_k[2], full[2])
    del calls[:]
    with torch.no_grad():
        y = degrade.blur_downsample(x, ker, 2, "bicubic")
    assert not y.requires_grad and _same_bits(y, full[0]) and calls == []


def test_clip_and_double_backward():
    g = torch.Generator().manual_seed(13)
    x, ker = (torch.rand(1, 3, 30, 30, generator=g) * 9 - 4).cuda(), torch.rand(1, 1, 5, 5, generator=g).cuda()
    ker = ker / ker.sum()
    plain = degrade.blur_downsample(x, ker, 2, "direct", border="symmetric")
    clipped = degrade.blur_downsample(x, ker, 2, "direct", border="symmetric", clip=True)
    assert float(plain.min()) < 0 and float(plain.max()) > 1 and torch.equal(clipped, plain.clamp(0, 1))
    blur = degrade.blur_downsample(x, ker, 1, "direct", border="symmetric").clamp(0, 1)            # bicubic clips the blur, not the result
    want = degrade.blur_downsample(blur, torch.ones(1, 1, 1, 1, device="cuda"), 2, "bicubic", border="symmetric")
    assert torch.equal(degrade.blur_downsample(x, ker, 2, "bicubic", border="symmetric", clip=True), want)
    xr = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="clip"):
        degrade.blur_downsample(xr, ker, 2, clip=True)
    y = degrade.blur_downsample(xr, ker, 2)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(y.sum(), xr, create_graph=True)


@pytest.mark.parametrize("down", ["Bicubic", "Direct"])
def test_elbo_sisr_hip_against_torch_on_the_device(down):
    """the inputs and bars of tests/test_loss.py::test_elbo_sisr_matches_reference_golden, degrade_impl="hip" against "torch" on the device"""
    G = json.load(open(os.path.join(GOLDEN, "loss_sisr.json")))
    n, sf, (hl, wl) = G["n"], G["sf"], G["lr_hw"]

    def run(impl):
        g = np.random.Generator(np.random.Philox(key=G["seed"]))
        mu = torch.from_numpy(g.random((n, 3, hl * sf, wl * sf), dtype=np.float32)).cuda().requires_grad_(True)
        sigma = torch.from_numpy(g.random((n, 1, 1, 1), dtype=np.float32) * 0.01 + 1e-4).cuda().requires_grad_(True)
        kinfo = torch.from_numpy(np.stack([g.random(n) * 3 + 0.5, g.random(n) * 3 + 0.5, g.random(n) * 1.2 - 0.6], 1).astype(np.float32)).cuda().requires_grad_(True)
        im_hr = torch.from_numpy(g.random((n, 3, hl * sf, wl * sf), dtype=np.float32)).cuda()
        im_lr = torch.from_numpy(g.random((n, 3, hl, wl), dtype=np.float32)).cuda()
        prior = torch.from_numpy(g.random((n, 1, 1, 1), dtype=np.float32) * 0.01 + 1e-4).cuda()
        kgt = torch.from_numpy(np.stack([g.random(n) * 3 + 0.5, g.random(n) * 3 + 0.5, g.random(n) * 1.2 - 0.6], 1).astype(np.float32)).cuda()
        alpha0 = 0.5 * torch.tensor([G["var_window"] ** 2], dtype=torch.float32).cuda()
        kappa0 = torch.tensor([G["kappa0"]]).cuda()
        torch.manual_seed(G["torch_seed"])
        out, det = loss.elbo_sisr(mu=mu, sigma_est=sigma, kinfo_est=kinfo, im_hr=im_hr, im_lr=im_lr, sigma_prior=prior, alpha0=alpha0,
                                  kinfo_gt=kgt, kappa0=kappa0, r2=G["r2"], eps2=G["eps2"], sf=sf, k_size=G["k_size"], penalty_K=G["penalty_K"],
                                  shift=False, downsampler=down, degrade_impl=impl)
        out.backward()
        return ([float(out)] + [float(v) for v in det[:7]], float(mu.grad.double().sum()), float(mu.grad.abs().max()),
                [float(v) for v in sigma.grad.reshape(-1)], [float(v) for v in kinfo.grad.reshape(-1)])

    want, got = run("torch"), run("hip")
    print(down, "torch", want, "\nhip", got)
    assert got[0] == pytest.approx(want[0], rel=2e-5)
    assert got[1] == pytest.approx(want[1], rel=1e-4) and got[2] == pytest.approx(want[2], rel=1e-4)
    assert got[3] == pytest.approx(want[3], rel=1e-4)
    assert got[4] == pytest.approx(want[4], rel=2e-3, abs=1e-4)


def _small_set5(count=2):
    files = sorted(glob.glob(os.path.join(GOLDEN, "set5", "*.bmp")), key=lambda f: (os.path.getsize(f), f))
    return files[:count]


@pytest.fixture(scope="module")
def eval_cases():
    """two Set5 fixtures x two of test_kernels(4): ground truth, kernel and the host degradation for both downsamplers (computed once)"""
    sf = 4
    kernels = sisr_eval.test_kernels(sf)
    out = []
    for f in _small_set5():
        gt = sisr_eval.modcrop(veval.imread_rgb_uint8(f), sf)
        im = veval.img_as_float32(gt)
        for kidx in (0, 5):
            out.append((im, kernels[kidx], {d: sisr_eval.degrade(im, kernels[kidx], sf, downsampler=d) for d in ("bicubic", "direct")}))
    return sf, out


@pytest.mark.parametrize("down", ["bicubic", "direct"])
def test_degrade_lr_against_the_host_degradation(eval_cases, down):
    sf, cases = eval_cases
    for im, kernel, host in cases:
        got = degrade.degrade_lr(im, kernel, sf, downsampler=down)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (1, 3) + host[down].shape[:2]
        x64 = torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[None])).double()
        k64 = torch.from_numpy(np.ascontiguousarray(kernel[::-1, ::-1]))[None, None]
        s = ref_op(x64.abs(), k64.abs(), sf, down, "symmetric", abs_taps=True)[0].permute(1, 2, 0).numpy()
        err = np.abs(got[0].permute(1, 2, 0).cpu().numpy().astype(np.float64) - host[down].astype(np.float64))
        bar = kernel.size * 2.0 ** -23 * s + 2.0 ** -23
        print(f"{down} {im.shape}: max err {err.max():.3e}, max err/bar {(err / bar).max():.3f}")
        assert (err <= bar).all()


def test_sisr_table_device_degrade_matches_host(tmp_path):
    sf = 4
    for f in _small_set5():
        shutil.copy(f, tmp_path / os.path.basename(f))
    spec = f"{tmp_path}:bmp"
    kernels = [sisr_eval.test_kernels(sf)[i] for i in (0, 5)]

    def stub(lr, s):
        """nearest x s in place of the network; an HWC array from the host degradation or a [1,3,h,w] tensor from the device's"""
        if isinstance(lr, torch.Tensor):
            assert lr.is_cuda and lr.dim() == 4 and lr.shape[:2] == (1, 3)
            return lr.repeat_interleave(s, 2).repeat_interleave(s, 3)
        return np.repeat(np.repeat(lr, s, 0), s, 1)

    host = sisr_eval.sisr_table(stub, [spec], sf, kernels=kernels, with_ssim=False)
    dev = sisr_eval.sisr_table(stub, [spec], sf, kernels=kernels, with_ssim=False, device_degrade=True, device_metrics=True)
    assert len(host) == len(dev) == 2
    for hr, dr in zip(host, dev):
        assert list(hr) == list(dr)
        assert all(hr[key] == dr[key] for key in ("dataset", "kernel", "images"))
        assert len(dr["per_image_psnr_y"]) == 2
        assert np.abs(np.array(hr["per_image_psnr_y"]) - np.array(dr["per_image_psnr_y"])).max() <= 0.01
        assert abs(hr["psnr_y"] - dr["psnr_y"]) <= 0.01
    # device degradation with the host metrics: the stub's tensor comes back to the host in the caller
    mixed = sisr_eval.sisr_table(lambda lr, s: stub(lr, s)[0].permute(1, 2, 0).cpu().numpy(), [spec], sf, kernels=kernels[:1], device_degrade=True,
                                 with_ssim=False)
    assert np.abs(np.array(mixed[0]["per_image_psnr_y"]) - np.array(host[0]["per_image_psnr_y"])).max() <= 0.01


@pytest.mark.parametrize("mode, sf", [("direct", 4), ("bicubic", 3)])
def test_graph_capture_replays_the_eager_result(monkeypatch, mode, sf):
    g = torch.Generator().manual_seed(14)
    x, ker = torch.rand(2, 3, 50, 67, generator=g).cuda(), torch.rand(2, 1, 21, 21, generator=g).cuda()
    degrade.warm_taps(50, 67, sf, x.device)                    # the tables are uploaded outside the capture
    eager = degrade.blur_downsample(x, ker, sf, mode)
    torch.cuda.synchronize()
    streams = []
    real = _native.stream_handle
    monkeypatch.setattr(_native, "stream_handle", lambda: (streams.append(real()), streams[-1])[1])
    graph = torch.cuda.CUDAGraph()
    with _native.capture_lock, torch.cuda.graph(graph):
        capture_stream = torch.cuda.current_stream().cuda_stream
        out = degrade.blur_downsample(x, ker, sf, mode)
    monkeypatch.undo()
    # every launch went to the one capturing stream: the graph is a chain, it has no parallel branches
    assert len(streams) == (1 if mode == "direct" else 3) and set(streams) == {capture_stream}
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out, eager)
    x.copy_(torch.rand(2, 3, 50, 67, generator=g))
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out, degrade.blur_downsample(x, ker, sf, mode))
