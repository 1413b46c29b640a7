"""The SISR training loop on the GPU (virnet_amd/fit.py fit_sisr; csrc/small.hip sft_backward_kernel<true> + sft_partials_reduce_kernel;
csrc/metrics.hip's float-Y mode; datagen.GeneralTestSet): the order-fixed SFT backward against autograd, against itself (two calls, an
image alone and inside a batch, NaN-filled outputs) and under the software red zone; the float-Y metric against its host definition; the
validation set against ``general_test_np`` (which tests/test_fit_sisr_host.py pins to the reference's ``GeneralTest``); one SISR step
twice; ``fit_sisr`` against the loop a user writes by hand with the reference's per-step host reads -- logged values, epoch means and
parameters bit for bit -- the bitwise resume, the absence of host synchronisation between two log reads and the validation stage against
the host pipeline."""
import functools
import glob
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from redzone import guarded
from virnet_amd import _native, datagen, elbo, fit, metrics, ops, schedule, sisr_eval, trainlog
from virnet_amd import eval as veval
from virnet_amd.networks import VIRAttResUNetSR
from virnet_amd.optim import ClipAdam
from virnet_amd.utils.synth import synth_state_dict

pytestmark = pytest.mark.gpu


def same_bits(a, b) -> bool:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the order-fixed SFT backward ------------------------------------------------------------------------------------------------------------
SFT_CASES = [(2, 5, 7, 96, True),            # hw 35: one chunk; c4 = 24, 10 pixel lanes, 16 idle threads
             (1, 32, 32, 4, False),          # hw 1024: exactly one chunk; c4 = 1
             (2, 33, 32, 160, True),         # hw 1056: two chunks
             (3, 41, 50, 224, False),        # hw 2050: three chunks, the last of 2 pixels
             (1, 48, 48, 1024, True)]        # c4 = 256: one pixel lane
SFT_IDS = ["hw35_c96", "hw1024_c4", "hw1056_c160", "hw2050_c224", "hw2304_c1024"]


@functools.lru_cache(maxsize=None)
def sft_case(n, h, w, c, with_res):
    """inputs and the autograd gradients (tests/test_sisr_train_gpu.py::test_sft_backward_kernel_vs_autograd's construction), computed once"""
    g = torch.Generator().manual_seed(40 + c + h)
    x = (torch.rand(n, h, w, c, generator=g) - 0.5).requires_grad_(True)
    mul = (0.3 + torch.rand(n, c, generator=g)).requires_grad_(True)
    add = (torch.rand(n, c, generator=g) - 0.5).requires_grad_(True)
    da = torch.rand(n, h, w, c, generator=g) - 0.5
    res = torch.rand(n, h, w, c, generator=g) - 0.5 if with_res else None
    torch.nn.functional.leaky_relu(x * mul[:, None, None, :] + add[:, None, None, :], 0.2).backward(da)
    ref = (x.grad + (res if with_res else 0), mul.grad.clone(), add.grad.clone())
    dev = dict(da=da.cuda(), x=x.detach().cuda(), mul=mul.detach().cuda(), add=add.detach().cuda(), res=None if res is None else res.cuda())
    return dev, ref


def _sft(t, sel=None):
    pick = (lambda v: v) if sel is None else (lambda v: None if v is None else v[sel].contiguous())
    return ops.sft_backward(pick(t["da"]), pick(t["x"]), pick(t["mul"]), pick(t["add"]), slope=0.2, res=pick(t["res"]))


@pytest.mark.parametrize("n,h,w,c,with_res", SFT_CASES, ids=SFT_IDS)
def test_sft_backward_ordered(n, h, w, c, with_res):
    t, (ref_dx, ref_dmul, ref_dadd) = sft_case(n, h, w, c, with_res)
    dx, dmul, dadd = _sft(t)
    e_dx, e_m, e_a = (float((got.cpu() - ref).abs().max()) for got, ref in ((dx, ref_dx), (dmul, ref_dmul), (dadd, ref_dadd)))
    print(f"hw {h * w} c {c}: dx err {e_dx:.2e}, dmul err {e_m:.2e} (|ref| {float(ref_dmul.abs().max()):.2f}), dadd err {e_a:.2e} "
          f"(|ref| {float(ref_dadd.abs().max()):.2f})")
    assert e_dx <= 1e-6                                                               # the bars of test_sft_backward_kernel_vs_autograd
    assert e_m <= 2e-5 * max(1.0, float(ref_dmul.abs().max()))
    assert e_a <= 2e-5 * max(1.0, float(ref_dadd.abs().max()))
    # two calls give equal bits
    again = _sft(t)
    assert all(same_bits(a, b) for a, b in zip((dx, dmul, dadd), again))
    # image i alone gives the bits it has inside the batch
    for i in range(n):
        alone = _sft(t, slice(i, i + 1))
        assert same_bits(alone[0][0], dx[i]) and same_bits(alone[1][0], dmul[i]) and same_bits(alone[2][0], dadd[i]), i
    # dmul / dadd handed in as NaN-filled buffers come back finite (and the same): nothing is accumulated onto them; dx is the
    # atomic entry's, bit for bit
    lib = _native.load()
    nan_m, nan_a = torch.full((n, c), float("nan"), device="cuda"), torch.full((n, c), float("nan"), device="cuda")
    dx2 = torch.empty_like(dx)
    part = torch.full((lib.virnet_sft_backward_scratch_bytes(n, h * w, c) // 4,), float("nan"), device="cuda")
    _native.check(lib.virnet_sft_backward_ordered(t["da"].data_ptr(), t["x"].data_ptr(), t["mul"].data_ptr(), t["add"].data_ptr(), _native.ptr(t["res"]),
                                                  0.2, dx2.data_ptr(), nan_m.data_ptr(), nan_a.data_ptr(), part.data_ptr(), n, h * w, c,
                                                  _native.stream_handle()), "sft_backward_ordered")
    assert bool(torch.isfinite(nan_m).all()) and bool(torch.isfinite(nan_a).all()) and bool(torch.isfinite(part).all())
    assert same_bits(nan_m, dmul) and same_bits(nan_a, dadd) and same_bits(dx2, dx)
    dx3, zm, za = torch.empty_like(dx), torch.zeros_like(dmul), torch.zeros_like(dadd)
    _native.check(lib.virnet_sft_backward(t["da"].data_ptr(), t["x"].data_ptr(), t["mul"].data_ptr(), t["add"].data_ptr(), _native.ptr(t["res"]), 0.2,
                                          dx3.data_ptr(), zm.data_ptr(), za.data_ptr(), n, h * w, c, _native.stream_handle()), "sft_backward")
    assert same_bits(dx3, dx)
    assert float((zm - dmul).abs().max()) <= 2e-5 * max(1.0, float(ref_dmul.abs().max()))      # (the atomic entry: same sums, free order)


@pytest.mark.parametrize("n,h,w,c,with_res", SFT_CASES[2:4], ids=SFT_IDS[2:4])
def test_sft_backward_ordered_stays_inside_its_buffers(n, h, w, c, with_res):
    """Inputs through ``g.input``; dx, dmul, dadd and the scratch come from ``ops.sft_backward``'s own ``torch.empty`` inside the guard, so
    all four lie between guard zones and start out as NaN patterns: no zone is touched, every output element is written, no NaN."""
    t, _ = sft_case(n, h, w, c, with_res)
    plain = _sft(t)
    torch.cuda.synchronize()
    with guarded() as g:
        inside = {k: (None if v is None else g.input(v)) for k, v in t.items()}
        before = len(g.arenas)
        out = _sft(inside)
        made = g.arenas[before:]
        assert sorted(a.nbytes for a in made) == sorted([n * h * w * c * 4, n * c * 4, n * c * 4, n * ((h * w + 1023) // 1024) * 2 * c * 4])
        g.check(out)
        assert all(g.home(o) is not None for o in out)
        part = max((a for a in made if a.shape == (n * ((h * w + 1023) // 1024) * 2 * c,)), key=lambda a: a.nbytes)
        assert part.unwritten_count(0, part.nbytes) == 0                                # the scratch is written in full
        assert all(same_bits(a, b) for a, b in zip(out, plain))


# ---- the float-Y metric ----------------------------------------------------------------------------------------------------------------------
def _float_pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(*shape, generator=g)
    mu = gt + 0.08 * torch.randn(*shape, generator=g) + 0.3 * (torch.rand(*shape, generator=g) - 0.5) * (torch.rand(*shape, generator=g) < 0.2)
    return (mu * 1.3 - 0.15).contiguous(), gt.contiguous()          # values beyond [0, 1] on both sides


def _host_float_y(mu, gt, border, with_ssim):
    """the test stage's host pipeline (util_image.batch_PSNR / batch_SSIM with ycbcr=True) from the definitions: bytes of the float Y"""
    ya, yb = veval.img_as_ubyte(metrics.rgb2y_float_np(mu)), veval.img_as_ubyte(metrics.rgb2y_float_np(gt))
    out = []
    for a, b in zip(ya[:, 0], yb[:, 0]):
        h, w = a.shape
        d = a[border:h - border, border:w - border].astype(np.int64) - b[border:h - border, border:w - border].astype(np.int64)
        out.append((int((d * d).sum()), d.size, veval.calculate_psnr(b, a, border), veval.calculate_ssim(b, a, border) if with_ssim else None))
    return out


@pytest.mark.parametrize("border", [0, 4, 9])
@pytest.mark.parametrize("shape", [(2, 3, 23, 37), (1, 3, 40, 40)], ids=["23x37", "40x40"])
def test_float_y_metric_is_the_host_definition(shape, border):
    mu, gt = _float_pair(shape, 11 + shape[2])
    with_ssim = min(shape[2:]) - 2 * border >= 11          # (23 x 37 cropped by 9 leaves 5 rows: no 11 x 11 window, on the host either)
    sse, cnt, ssim = metrics.psnr_ssim(mu.cuda(), gt.cuda(), border=border, ycbcr="float", with_ssim=with_ssim)
    psnrs, ssims = metrics.to_floats(sse, cnt, ssim)
    for i, (h_sse, h_cnt, h_psnr, h_ssim) in enumerate(_host_float_y(mu.numpy(), gt.numpy(), border, with_ssim)):
        assert (int(sse[i]), int(cnt[i])) == (h_sse, h_cnt)
        assert psnrs[i] == h_psnr                                                       # the host's double
        if with_ssim:
            print(f"{shape} border {border} image {i}: SSIM error {abs(ssims[i] - h_ssim):.2e}")
            assert abs(ssims[i] - h_ssim) <= 1e-10
    # not the evaluation scripts' metric: Y of the quantised RGB image gives other bytes
    other = metrics.psnr_ssim(mu.cuda(), gt.cuda(), border=border, ycbcr=True, with_ssim=with_ssim)
    assert not torch.equal(other[0], sse)
    with pytest.raises(TypeError, match="float32 images"):
        metrics.psnr_ssim(mu.cuda(), (gt * 255).to(torch.uint8).cuda(), border=border, ycbcr="float")


@pytest.mark.parametrize("ycbcr", [False, True], ids=["rgb", "y"])
def test_existing_metric_modes_are_unchanged(ycbcr):
    """ycbcr = False / True: the exact error sums of the host definitions they had (eval.img_as_ubyte, eval.rgb2y_uint8), SSIM within
    1e-10 of eval.calculate_ssim, and the same bits from call to call."""
    mu, gt = _float_pair((2, 3, 23, 37), 5)
    a = metrics.psnr_ssim(mu.cuda(), gt.cuda(), border=4, ycbcr=ycbcr)
    b = metrics.psnr_ssim(mu.cuda(), gt.cuda(), border=4, ycbcr=ycbcr)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    psnrs, ssims = metrics.to_floats(*a)
    for i in range(2):
        qa = veval.img_as_ubyte(mu[i].numpy().transpose(1, 2, 0))
        qb = veval.img_as_ubyte(gt[i].numpy().transpose(1, 2, 0))
        want = veval.calculate_psnr_y(qb, qa, 4) if ycbcr else veval.calculate_psnr(qb, qa, 4)
        assert psnrs[i] == want and abs(ssims[i] - veval.calculate_ssim(qb, qa, 4, ycbcr=ycbcr)) <= 1e-10


def test_float_y_metric_stays_inside_its_buffers():
    mu, gt = _float_pair((2, 3, 23, 37), 7)
    plain = metrics.psnr_ssim(mu.cuda(), gt.cuda(), border=4, ycbcr="float")
    torch.cuda.synchronize()
    with guarded() as g:
        out = metrics.psnr_ssim(g.input(mu.cuda()), g.input(gt.cuda()), border=4, ycbcr="float")
        g.check(out)
        assert all(g.home(o) is not None for o in out) and all(same_bits(a, b) for a, b in zip(out, plain))


# ---- GeneralTestSet --------------------------------------------------------------------------------------------------------------------------
def _crops():
    g = load_golden("general_test")
    return [g["u8_0"], g["u8_1"]]


@pytest.mark.parametrize("sf,down,shift", [(2, "direct", False), (4, "bicubic", False), (2, "bicubic", True)],
                         ids=["sf2_direct", "sf4_bicubic", "sf2_bicubic_shifted"])
def test_general_test_set_is_the_definition(sf, down, shift):
    """``shift``: the half-pixel centre makes the kernel asymmetric, so applying it in the wrong direction (the set hands the kernel to
    ``synthesize_lr`` as the dataset makes it, to be applied as a true convolution) would miss the bar by orders of magnitude."""
    images = _crops()
    want = datagen.general_test_np(images, sf, 21, shift, down, "Gaussian")
    vs = datagen.GeneralTestSet(datagen.ImagePool(images, "cuda"), sf, kernel_shift=shift, downsampler=down)
    assert len(vs) == 2 and vs.groups() == [[0], [1]] and np.array_equal(vs.noise_np, datagen.general_noise([(44, 60), (60, 44)], sf))
    for i, (w_hr, w_lr, w_k) in enumerate(want):
        im_hr, im_lr, kinfo = vs.batch([i])
        assert im_hr.shape == (1,) + w_hr.shape and im_lr.shape == (1,) + w_lr.shape and kinfo.shape == (1, 3)
        assert same_bits(im_hr[0], w_hr) and same_bits(kinfo[0], w_k)
        # the bar derived in tests/test_datagen_gpu.py:153-158: twice k^2 2^-23 times the blur (image and kernel are non-negative), and one
        # more rounding for the noise's sum
        blur_max = float(sisr_eval.synthesize_lr_np(np.ascontiguousarray(w_hr.transpose(1, 2, 0)),
                                                    sisr_eval.anisotropic_gaussian_kernel(21, sf, 1.6 ** 2, 1.6 ** 2, 0.0, shift)[0], sf,
                                                    np.zeros(w_lr.shape[1:] + (3,), np.float32), 0.0, 0, down)[1].max())
        bar = 2 * 21 * 21 * 2.0 ** -23 * blur_max + 2.0 ** -23
        err = float(np.abs(im_lr[0].cpu().numpy() - w_lr).max())
        print(f"sf {sf} {down} image {i}: im_lr max err {err:.2e}, bar {bar:.2e}")
        assert err <= bar
        # batch twice gives the same tensors without a launch: the resident stack's views, from the cache
        again = vs.batch([i])
        assert all(a is b for a, b in zip(again, (im_hr, im_lr, kinfo)))
    with pytest.raises(ValueError, match="one shape"):
        vs.batch([0, 1])


def test_general_test_set_jpeg_and_same_shape_batches():
    """Against ``general_test_np`` with ``noise_type="JPEG"``, end to end: within one byte / 255 on at most the share of pixels that
    tests/test_jpeg_gpu.py allows ``synthesize_lr``'s JPEG tail -- and that file allows none: it holds the tail to the host codec bit for
    bit.  So the bar is a share of zero, on all three images (every value of a round trip's output is a byte / 255 formed by the same fp32
    product on both sides, so "no byte differs" and "equal floats" are one statement).  Also the tail on its own, as that file spells it:
    the JPEG set equals the host codec on the device's own pre-JPEG image, the Gaussian set's."""
    images = _crops()
    images = images + [images[0][::-1].copy()]                                          # a second 44 x 60 image: one group of two
    pool = datagen.ImagePool(images, "cuda")
    gauss, jpeg = datagen.GeneralTestSet(pool, 2, downsampler="direct"), datagen.GeneralTestSet(pool, 2, downsampler="direct", noise_type="JPEG")
    assert gauss.groups() == jpeg.groups() == [[0, 2], [1]]
    want = datagen.general_test_np(images, 2, 21, False, "direct", "JPEG")
    for i in range(3):
        lr_g, lr_j = gauss.batch([i])[1][0], jpeg.batch([i])[1][0]
        tail = veval.jpeg_compress(np.ascontiguousarray(lr_g.cpu().numpy().transpose(1, 2, 0)), 40)
        assert same_bits(lr_j, np.ascontiguousarray(tail.transpose(2, 0, 1)))
        diff = np.abs(lr_j.cpu().numpy() - want[i][1]) * 255
        share = float((diff > 0.5).mean())
        print(f"image {i}: against general_test_np end to end: {share:.4%} of the values differ, by at most {diff.max():.1f} / 255")
        assert diff.max() <= 1.0 and share == 0.0 and same_bits(lr_j, want[i][1])
        assert same_bits(jpeg.batch([i])[0], gauss.batch([i])[0])
    both = gauss.batch([0, 2])
    assert both[0].shape == (2, 3, 44, 60) and same_bits(both[1][1], gauss.batch([2])[1][0]) and gauss.batch([0, 2])[0] is both[0]
    swapped = gauss.batch([2, 0])
    assert same_bits(swapped[1][0], both[1][1]) and gauss.batch([2, 0])[1] is swapped[1]


# ---- the step and the loop -------------------------------------------------------------------------------------------------------------------
# SMALL of tests/test_sisr_train_gpu.py, restated
SMALL = dict(im_chn=3, sigma_chn=1, kernel_chn=3, n_feat=[64, 96], dep_S=3, dep_K=2, noise_cond=True, kernel_cond=True, n_resblocks=1,
             extra_mode="Both", noise_avg=True)
# the reference's keys as configs/sisr_x2.json spells them (booleans as strings), at 48 x 48 HR patches: LR 24 x 24, so KNet's quarter-
# resolution map has 6 rows (every weight gradient takes the f16 route) and RNet's top level 48 x 48 = 2304 pixels = three chunks
CFG = dict(im_chn=3, sigma_chn=1, hr_size=48, batch_size=4, epochs=2, lr=2e-4, lr_min=1e-6, print_freq=2, sf=2, k_size=21, add_jpeg="False",
           kernel_shift="False", downsampler="Bicubic", noise_level=[0.01, 15], noise_jpeg=[0.01, 10], eps2=1e-5, r2=1e-4, var_window=9, kappa0=50,
           penalty_K=[0.02, 2], clip_grad_R=5e2, clip_grad_S=1e2, clip_grad_K=5e2, steps_per_epoch=3)


def _net(noise_avg=True):
    net = VIRAttResUNetSR(**dict(SMALL, noise_avg=noise_avg))
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=5), strict=True)
    return net.cuda()


@pytest.fixture(scope="module")
def pool():
    files = sorted(glob.glob(os.path.join(GOLDEN, "cbsd68", "*.png")))[:4]
    assert len(files) == 4
    return datagen.ImagePool([veval.imread_rgb_uint8(f) for f in files], "cuda")


@pytest.fixture(scope="module")
def val():
    return datagen.GeneralTestSet(datagen.ImagePool(_crops(), "cuda"), 2)


def hand_loop(net, pool, cfg, epochs=None):
    """The loop a user writes by hand from the package's pieces, with the reference's eight host reads per step (train_SISR.py:185-243)."""
    c = fit.read_sisr_config(cfg)
    named = list(net.named_parameters())
    sets = [[p for n, p in named if key in n.lower()] for key in ("rnet", "snet", "knet")]
    opt = ClipAdam(net.parameters(), lr=c["lr"], clip=list(zip(sets, (c["clip_grad_R"], c["clip_grad_S"], c["clip_grad_K"]))))
    lrs = schedule.cosine(c["lr"], c["lr_min"], c["epochs"])
    alpha0 = 0.5 * torch.tensor([c["var_window"] ** 2], dtype=torch.float32).cuda()
    kappa0 = torch.tensor([c["kappa0"]], dtype=torch.float32).cuda()
    b, hr, sf, num_iter = c["batch_size"], c["hr_size"], c["sf"], c["steps_per_epoch"]
    rows, means = [], []
    for epoch in range(c["epochs"] if epochs is None else epochs):
        rng = random.Random(epoch * 1000)
        torch.manual_seed(epoch * 1000)
        for group in opt.param_groups:
            group["lr"] = lrs[epoch]
        net.train()
        per_epoch = {x: 0 for x in ("Loss", "lh", "KLR", "KLS", "KLK")}
        for ii in range(num_iter):
            prm = datagen.draw_sisr_params(rng, pool, b, hr, sf, c["noise_level"], c["add_jpeg"], c["noise_jpeg"])
            im_hr, im_lr, im_blur, kinfo_gt, nlevel = datagen.sisr_batch(pool, prm, hr, sf, c["k_size"], seed=epoch * 1000, downsampler=c["downsampler"],
                                                                         shift=c["kernel_shift"], base_id=ii * b)
            sigma_prior = elbo.noise_estimate(im_lr, im_blur, c["var_window"]) if c["add_jpeg"] else nlevel
            opt.zero_grad()
            mu, kinfo_est, sigma_est = net(im_lr, sf)
            loss, detail = elbo.elbo_sisr(mu=mu, sigma_est=sigma_est, kinfo_est=kinfo_est, im_hr=im_hr, im_lr=im_lr, sigma_prior=sigma_prior,
                                          alpha0=alpha0, kinfo_gt=kinfo_gt, kappa0=kappa0, r2=c["r2"], eps2=c["eps2"], sf=sf, k_size=c["k_size"],
                                          penalty_K=c["penalty_K"], downsampler=c["downsampler"], shift=c["kernel_shift"])
            loss.backward()
            opt.step()
            for key, v in zip(per_epoch, (loss, detail[0], detail[1], detail[2], detail[3])):
                per_epoch[key] += v.item() / num_iter
            rows.append([loss.item(), detail[0].item(), detail[1].item(), detail[2].item(), detail[3].item()] + opt.grad_norms.tolist())
        means.append(per_epoch)
    return np.asarray(rows, dtype=np.float32), means, opt


def _same_state(net_a, net_b):
    return all(torch.equal(a, b) for a, b in zip(net_a.state_dict().values(), net_b.state_dict().values()))


def _same_adam(opt_a, opt_b):
    sa, sb = opt_a.state_dict()["state"], opt_b.state_dict()["state"]
    return sa.keys() == sb.keys() and len(sa) > 0 and all(
        float(sa[k]["step"]) == float(sb[k]["step"]) and torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"])
        and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"]) for k in sa)


def test_one_step_twice_gives_the_same_bits(pool):
    """One SISR step from the same state and seeds, twice: every gradient and every parameter bitwise equal.  Every level's map has at
    least 5 rows here (24, 12 and KNet's 6), so every weight gradient takes the f16 route, whose sums are order-fixed; the SFT backward's
    dmul / dadd -- three chunks per image at the top level -- are order-fixed since virnet_sft_backward_ordered."""
    c = fit.read_sisr_config(CFG)
    runs = []
    for _ in range(2):
        net = _net().train()
        opt = fit.sisr_optimizer(net, c)
        torch.manual_seed(0)
        fit.sisr_train_step(net, opt, pool, c, random.Random(0), 0, 0, 0.5 * torch.tensor([81.0]).cuda(), torch.tensor([50.0]).cuda())
        runs.append((net, {k: p.grad.clone() for k, p in net.named_parameters()}))
    differ = [k for k in runs[0][1] if not torch.equal(runs[0][1][k], runs[1][1][k])]
    print("gradients that differ between two identical steps:", differ)
    assert not differ
    assert all(bool(torch.isfinite(g).all()) for g in runs[0][1].values()) and _same_state(runs[0][0], runs[1][0])


@pytest.fixture(scope="module")
def sisr_run(tmp_path_factory, pool, val):
    """fit_sisr for 2 epochs x 3 steps with validation and checkpoints: shared (read-only) by the tests below"""
    save_dir = tmp_path_factory.mktemp("fit_sisr")
    net = _net()
    lines = []
    out = fit.fit_sisr(net, pool, CFG, val=val, save_dir=save_dir, log=lines.append)
    return dict(net=net, out=out, lines=lines, save_dir=save_dir)


def test_fit_sisr_is_the_hand_written_loop_bit_for_bit(sisr_run, pool):
    out, lines = sisr_run["out"], sisr_run["lines"]
    ref_net = _net()
    rows, means, opt = hand_loop(ref_net, pool, CFG)
    assert out["rows"].shape == (6, 8) and out["rows"].dtype == np.float32 and np.array_equal(out["rows"].view(np.uint32), rows.view(np.uint32))
    assert out["train"] == means                                                   # the epoch means: the same Python doubles
    assert _same_state(sisr_run["net"], ref_net) and _same_adam(out["optimizer"], opt)
    assert out["lr"] == schedule.cosine(2e-4, 1e-6, 2) and out["epoch_start"] == 0 and out["step"] == 4
    assert np.isfinite(out["rows"]).all() and not np.array_equal(rows[0], rows[3])
    # the reference's lines, the whole transcript: per epoch steps 1 and 2 of 3 are printed (ii == 0, print_freq 2), then the epoch line, a
    # rule, the test stage's summary (two validation images: no every-third-image line; the mean is the running sum over 2), a rule and
    # the time line (its figure is not compared)
    took, want = "This epoch take time ", []
    for e in range(2):
        want += [fit.sisr_train_line(e, 2, ii, 3, rows[3 * e + ii], out["lr"][e]) for ii in (0, 1)]
        want += [fit.sisr_epoch_line([means[e][k] for k in ("Loss", "lh", "KLR", "KLS", "KLK")]), "-" * 105]
        psnrs, ssims = out["val_images"]["Gaussian"][e]
        want += [fit.sisr_summary_line("Gaussian", (psnrs[0] + psnrs[1]) / 2, (ssims[0] + ssims[1]) / 2), "-" * 60, took]
    assert [line[:len(took)] if line.startswith(took) else line for line in lines] == want
    assert lines[0].startswith("[Epoch:  1/2  ] train:00001/00003, lh:") and lines[7].startswith("[Epoch:  2/2  ] train:00001/00003, lh:")
    assert all(float(lines[k][len(took):]) >= 0.0 for k in (6, 13)) and len(psnrs) == len(ssims) == 2


def test_a_sisr_checkpoint_restores_parameters_and_adam_state_bit_for_bit(sisr_run):
    path = sisr_run["out"]["checkpoints"][1]
    ckpt = torch.load(path, map_location="cpu")
    assert set(ckpt) == {"epoch", "step", "step_img", "model_state_dict", "optimizer_state_dict"} and ckpt["epoch"] == 2 and ckpt["step"] == 5
    assert ckpt["step_img"] == {"train": 0, "Gaussian": 0}
    net = _net()
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
    opt = fit.sisr_optimizer(net, fit.read_sisr_config(dict(CFG, lr=1.0)))
    assert fit.load_checkpoint(path, net, opt, map_location="cuda")["epoch"] == 2
    assert _same_state(net, sisr_run["net"]) and _same_adam(opt, sisr_run["out"]["optimizer"])
    assert opt.param_groups[0]["lr"] == sisr_run["out"]["lr"][1]


def test_sisr_resume_is_bitwise(sisr_run, pool, tmp_path):
    """Two epochs straight == one epoch, checkpoint, resume, one epoch: bitwise in the logged rows, parameters and Adam state."""
    net = _net()
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()                                                              # (everything must come from the checkpoint)
    straight = sisr_run["out"]
    out = fit.fit_sisr(net, pool, CFG, resume=straight["checkpoints"][0], save_dir=tmp_path, log=lambda s: None)
    assert out["epoch_start"] == 1 and out["lr"] == straight["lr"][1:] and out["psnr"] == {}
    assert np.array_equal(out["rows"].view(np.uint32), straight["rows"][3:].view(np.uint32))
    assert out["train"] == straight["train"][1:] and _same_state(net, sisr_run["net"]) and _same_adam(out["optimizer"], straight["optimizer"])
    final_a, final_b = torch.load(out["checkpoints"][0], map_location="cpu"), torch.load(straight["checkpoints"][1], map_location="cpu")
    assert final_a["epoch"] == final_b["epoch"] == 2
    assert all(torch.equal(final_a["model_state_dict"][k], v) for k, v in final_b["model_state_dict"].items())


def test_no_host_synchronisation_between_two_sisr_log_reads(pool):
    c = fit.read_sisr_config(CFG)
    net = _net().train()
    opt = fit.sisr_optimizer(net, c)
    alpha0, kappa0 = 0.5 * torch.tensor([81.0]).cuda(), torch.tensor([50.0]).cuda()
    log = trainlog.StepLog(fit.SISR_LOG_NAMES, 8, 3)
    rng = random.Random(0)
    torch.manual_seed(0)
    for ii in range(2):                                                            # the warm-up: plans, packed weights, cached tables
        fit.sisr_train_step(net, opt, pool, c, rng, 0, ii, alpha0, kappa0, log)
    assert log.read()[0].shape == (2, 8)
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for ii in range(2, 5):
            fit.sisr_train_step(net, opt, pool, c, rng, 0, ii, alpha0, kappa0, log)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    rows, _ = log.read()
    assert rows.shape == (3, 8) and np.isfinite(rows).all()


def test_sisr_validation_stage_equals_the_host_pipeline(sisr_run, val):
    """On the same ``mu``: PSNR is the host's double (batch_PSNR's bytes: img_as_ubyte of the float Y, border sf**2), SSIM within 1e-10."""
    net, out = sisr_run["net"], sisr_run["out"]
    net.eval()
    psnrs, ssims = [], []
    with torch.no_grad():
        for i in range(len(val)):
            im_hr, im_lr, _ = val.batch([i])
            mu = net(im_lr, 2)[0]
            (_, _, psnr, ssim), = _host_float_y(mu.cpu().numpy(), im_hr.cpu().numpy(), 4, True)
            psnrs.append(psnr)
            ssims.append(ssim)
    got_psnr, got_ssim = out["val_images"]["Gaussian"][-1]
    print("psnr", got_psnr, psnrs, "ssim", got_ssim, ssims)
    assert got_psnr == psnrs and max(abs(a - b) for a, b in zip(got_ssim, ssims)) <= 1e-10
    assert out["psnr"]["Gaussian"][-1] == (psnrs[0] + psnrs[1]) / 2 and abs(out["ssim"]["Gaussian"][-1] - (ssims[0] + ssims[1]) / 2) <= 1e-10
    assert len(out["psnr"]["Gaussian"]) == 2 and sisr_run["lines"][-3].startswith("Noise: Gaussian, test: PSNR=")


def test_fit_sisr_with_jpeg_is_its_hand_written_loop(pool):
    """add_jpeg: the net is built with noise_avg=False (train_SISR.py:87), the prior is noise_estimate(im_lr, im_blur, var_window) and some
    samples end in the JPEG round trip.  Two steps: bitwise the hand-written loop, and finite."""
    cfg = dict(CFG, add_jpeg="True", epochs=1, steps_per_epoch=2)
    with pytest.raises(ValueError, match="noise_avg=False"):
        fit.fit_sisr(_net(), pool, cfg, log=lambda s: None)
    net, ref_net = _net(False), _net(False)
    out = fit.fit_sisr(net, pool, cfg, log=lambda s: None)
    rows, means, _ = hand_loop(ref_net, pool, cfg)
    assert out["rows"].shape == (2, 8) and np.array_equal(out["rows"].view(np.uint32), rows.view(np.uint32)) and np.isfinite(rows).all()
    assert out["train"] == means and _same_state(net, ref_net)
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
