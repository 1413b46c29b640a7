"""Device metrics (virnet_amd/metrics.py, csrc/metrics.hip) against their host definition, virnet_amd/eval.py:

  * quantisation, luma, the integer squared-error sum and therefore PSNR: exact (``==``);
  * SSIM: |device - host| <= 1e-10.  Both sides are fp64 and differ only in summation order; the worst term is E[a^2], at most 22
    roundings of values <= 65 025 (<= 1.6e-10 absolute) entering a factor whose denominator is >= C2 = 58.5: ~1e-11 worst case, the bar
    is ten times that;
  * luma on the 194 RGB triples whose exact value ends in .5 may differ by 1 from a host whose dot product rounds the other way; every
    comparison in Y mode therefore checks the planes first and, if they differ there, feeds the device's planes to the host metric.
"""
import ctypes
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from virnet_amd import _native, eval as veval, metrics, sisr_eval
from virnet_amd.utils.synth import synth_state_dict

pytestmark = pytest.mark.gpu
SSIM_TOL = 1e-10
BORDERS = (0, 4, 16)


def nchw(im_hwc):
    return torch.from_numpy(np.ascontiguousarray(im_hwc.transpose(2, 0, 1)))


def hwc(t):
    return np.ascontiguousarray(t.cpu().numpy().transpose(1, 2, 0))


def pair(h, w, seed, sigma=20.0):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    a = (a // 4 + np.linspace(0, 190, w, dtype=np.float64)[None, :, None]).astype(np.uint8)        # structure + texture
    b = np.clip(np.rint(a.astype(np.float64) + rng.standard_normal(a.shape) * sigma), 0, 255).astype(np.uint8)
    return a, b


def tie_mask(r, g, b):
    return (2 * (65481 * r.astype(np.int64) + 128553 * g.astype(np.int64) + 24966 * b.astype(np.int64))) % 510000 == 255000


def host_planes(im_hwc, ycbcr):
    """The metric planes of an image [h,w,c]; in Y mode the device's planes stand in when they differ from the host's on tie pixels."""
    if not ycbcr:
        return im_hwc
    y_host = veval.rgb2y_uint8(im_hwc)
    y_dev = metrics.rgb2y(nchw(im_hwc)[None].cuda())[0, 0].cpu().numpy()
    if np.array_equal(y_host, y_dev):
        return y_host
    diff = y_host != y_dev
    ties = tie_mask(im_hwc[..., 0], im_hwc[..., 1], im_hwc[..., 2])
    assert not (diff & ~ties).any(), "device Y differs from eval.rgb2y_uint8 off the tie triples"
    assert np.abs(y_host.astype(int) - y_dev.astype(int)).max() <= 1
    print(f"Y planes differ on {int(diff.sum())} tie pixel(s): host metric computed from the device's planes")
    return y_dev


def host_numbers(a_hwc, b_hwc, border, ycbcr, with_ssim=True):
    pa, pb = host_planes(a_hwc, ycbcr), host_planes(b_hwc, ycbcr)
    h, w = pa.shape[:2]
    ca, cb = pa[border:h - border, border:w - border].astype(np.int64), pb[border:h - border, border:w - border].astype(np.int64)
    return (int(((ca - cb) ** 2).sum()), int(ca.size), veval.calculate_psnr(pa, pb, border),
            veval.calculate_ssim(pa, pb, border) if with_ssim else None)


def check_batch(pairs, border, ycbcr, label):
    """Device results for a list of equally sized uint8 HWC pairs, as a batch and one by one, against the host."""
    h, w = pairs[0][0].shape[:2]
    ssim_ok = min(h, w) - 2 * border >= 11
    ta = torch.stack([nchw(a) for a, _ in pairs]).cuda()
    tb = torch.stack([nchw(b) for _, b in pairs]).cuda()
    if not ssim_ok:
        with pytest.raises(ValueError, match="smaller than the 11x11 SSIM window"):
            metrics.psnr_ssim(ta, tb, border=border, ycbcr=ycbcr)
    sse, cnt, ssim = metrics.psnr_ssim(ta, tb, border=border, ycbcr=ycbcr, with_ssim=ssim_ok)
    one = metrics.psnr_ssim(ta[:1], tb[:1], border=border, ycbcr=ycbcr, with_ssim=ssim_ok)
    psnrs, ssims = metrics.to_floats(sse, cnt, ssim)
    assert int(one[0][0]) == int(sse[0]) and int(one[1][0]) == int(cnt[0])
    if ssim_ok:
        assert one[2].view(torch.int64)[0].item() == ssim.view(torch.int64)[0].item(), "batch of 1 and batch of 5 give different SSIM bits"
    worst = 0.0
    for i, (a, b) in enumerate(pairs):
        h_sse, h_cnt, h_psnr, h_ssim = host_numbers(a, b, border, ycbcr, ssim_ok)
        assert int(sse[i]) == h_sse and int(cnt[i]) == h_cnt, (label, i, int(sse[i]), h_sse)
        assert psnrs[i] == h_psnr, (label, i, psnrs[i], h_psnr)
        if ssim_ok:
            err = abs(ssims[i] - h_ssim)
            worst = max(worst, err)
            assert err <= SSIM_TOL, (label, i, ssims[i], h_ssim, err)
    print(f"{label}: {len(pairs)} image(s), worst SSIM error {worst:.2e}")


# ---- 1. quantise ---------------------------------------------------------------------------------------------------------------------
def test_quantise_matches_img_as_ubyte_on_every_boundary():
    k = np.arange(256, dtype=np.float64)
    base = np.concatenate([(k / 255.0).astype(np.float32), ((k + 0.5) / 255.0).astype(np.float32)])
    vals = [base]
    for _ in range(2):
        vals.append(np.nextafter(vals[-1], np.float32(2.0)))
    down = base
    for _ in range(2):
        down = np.nextafter(down, np.float32(-2.0))
        vals.append(down)
    rng = np.random.default_rng(11)
    tiny = np.float32(np.finfo(np.float32).tiny)
    vals += [np.array([0.0, -0.0, 1.0, -1.0, 2.0, -1e-30, 1e30, -1e30, np.inf, -np.inf, tiny, -tiny, tiny / 2, -tiny / 2, 1e-45, -1e-45,
                       1.0000001, 0.99999994, 0.5, 0.49999997, 0.50000006], dtype=np.float32),
             rng.uniform(-0.25, 1.25, size=200001).astype(np.float32),
             rng.standard_normal(70001).astype(np.float32)]
    x = np.concatenate(vals).astype(np.float32)
    for off in (0, 1, 3):                                    # aligned (16-byte loads) and misaligned starts, length not a multiple of 4
        xs = x[off:]
        dev = metrics.to_uint8(torch.from_numpy(x).cuda()[off:])
        assert np.array_equal(dev.cpu().numpy().reshape(-1), veval.img_as_ubyte(xs)), off
    nan = metrics.to_uint8(torch.full((5,), float("nan")).cuda())
    assert nan.cpu().tolist() == [0] * 5                     # documented: NaN -> 0


# ---- 2. luma, exhaustive ---------------------------------------------------------------------------------------------------------------
def test_luma_all_2_24_triples():
    idx = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    r, g, b = (idx >> 16).astype(np.uint8), ((idx >> 8) & 255).astype(np.uint8), (idx & 255).astype(np.uint8)
    rgb = np.stack([r, g, b], axis=-1)
    ties = tie_mask(r, g, b)
    assert int(ties.sum()) == 194
    y_host = veval.rgb2y_uint8(rgb)
    y_dev = metrics.rgb2y(nchw(rgb)[None].cuda())[0, 0].cpu().numpy()
    assert np.array_equal(y_dev[~ties], y_host[~ties])
    d = np.abs(y_dev[ties].astype(int) - y_host[ties].astype(int))
    print(f"luma: {int((d != 0).sum())} of the 194 tie triples differ from eval.rgb2y_uint8")
    assert d.max() <= 1


# ---- 3 + 4. PSNR and SSIM --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ycbcr", [False, True], ids=["rgb", "y"])
@pytest.mark.parametrize("border", BORDERS)
def test_psnr_ssim_sizes_and_batches(border, ycbcr):
    sizes = [(11 + 2 * border, 11 + 2 * border), (481, 321), (321, 481), (256, 256), (37, 53)]
    for (h, w) in sizes:
        pairs = [pair(h, w, seed=100 * h + w + i, sigma=5.0 + 10.0 * i) for i in range(5)]
        check_batch(pairs, border, ycbcr, f"{h}x{w} border {border} {'Y' if ycbcr else 'RGB'}")


@pytest.mark.parametrize("ycbcr", [False, True], ids=["rgb", "y"])
@pytest.mark.parametrize("border", BORDERS)
def test_psnr_ssim_special_images(border, ycbcr):
    h, w = 75, 91
    a, _ = pair(h, w, seed=5)
    zeros, full = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    grey = np.full((h, w, 3), 77, np.uint8)
    grey2 = np.full((h, w, 3), 78, np.uint8)
    pairs = [(a, a), (zeros, full), (grey, grey), (grey, grey2), (zeros, zeros)]
    check_batch(pairs, border, ycbcr, f"special border {border} {'Y' if ycbcr else 'RGB'}")
    ta = torch.stack([nchw(x) for x, _ in pairs]).cuda()
    tb = torch.stack([nchw(y) for _, y in pairs]).cuda()
    psnrs, ssims = metrics.to_floats(*metrics.psnr_ssim(ta, tb, border=border, ycbcr=ycbcr))
    assert psnrs[0] == float("inf") and psnrs[2] == float("inf") and abs(ssims[0] - 1.0) <= SSIM_TOL and abs(ssims[2] - 1.0) <= SSIM_TOL
    if not ycbcr:
        assert psnrs[1] == 0.0                               # mse = 255^2


def test_psnr_ssim_golden_images_with_seeded_noise():
    rng = np.random.default_rng(2024)
    for path, border, ycbcr in [(sorted(glob.glob(os.path.join(GOLDEN, "cbsd68", "*.png")))[0], 0, False),
                                (sorted(glob.glob(os.path.join(GOLDEN, "set5", "*.bmp")))[0], 16, True)]:
        gt = veval.imread_rgb_uint8(path)
        noisy = veval.img_as_ubyte(veval.img_as_float32(gt) + (rng.standard_normal(gt.shape) * (25 / 255.0)).astype(np.float32))
        check_batch([(noisy, gt)], border, ycbcr, os.path.basename(path))
        check_batch([(noisy, gt)], border, not ycbcr, os.path.basename(path))


def test_single_channel_inputs():
    a, b = pair(64, 80, seed=9)
    ta, tb = nchw(a)[None, :1].contiguous().cuda(), nchw(b)[None, :1].contiguous().cuda()
    sse, cnt, ssim = metrics.psnr_ssim(ta, tb, border=3)
    psnrs, ssims = metrics.to_floats(sse, cnt, ssim)
    assert psnrs[0] == veval.calculate_psnr(a[..., 0], b[..., 0], 3)
    assert abs(ssims[0] - veval.calculate_ssim(a[..., 0], b[..., 0], 3)) <= SSIM_TOL


# ---- 5. float inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ycbcr", [False, True], ids=["rgb", "y"])
def test_float_inputs_are_quantised_on_load(ycbcr):
    g = torch.Generator().manual_seed(4)
    mu = (torch.rand(3, 3, 123, 77, generator=g) * 1.3 - 0.15).cuda()
    gt = torch.randint(0, 256, (3, 3, 123, 77), generator=g, dtype=torch.uint8).cuda()
    direct = metrics.psnr_ssim(mu, gt, border=4, ycbcr=ycbcr)
    staged = metrics.psnr_ssim(metrics.to_uint8(mu), gt, border=4, ycbcr=ycbcr)
    swapped = metrics.psnr_ssim(metrics.to_uint8(mu), gt.float() / 255.0, border=4, ycbcr=ycbcr)     # k/255 in fp32 quantises back to k
    for d, s, w in zip(direct, staged, swapped):
        assert torch.equal(d.view(torch.int64), s.view(torch.int64)) and torch.equal(d.view(torch.int64), w.view(torch.int64))
    with torch.inference_mode():
        inf = metrics.psnr_ssim(mu, gt, border=4, ycbcr=ycbcr)
    assert torch.equal(inf[2].view(torch.int64), direct[2].view(torch.int64))
    req = mu.clone().requires_grad_(True)
    out = metrics.psnr_ssim(req * 1.0, gt, border=4, ycbcr=ycbcr)
    assert not out[2].requires_grad and torch.equal(out[0], direct[0])


# ---- 6. reproducibility ----------------------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_independent_of_the_batch():
    pairs = [pair(481, 321, seed=40 + i, sigma=8.0 * (i + 1)) for i in range(5)]
    ta = torch.stack([nchw(a) for a, _ in pairs]).cuda()
    tb = torch.stack([nchw(b) for _, b in pairs]).cuda()
    for ycbcr in (False, True):
        first = metrics.psnr_ssim(ta, tb, ycbcr=ycbcr)
        again = metrics.psnr_ssim(ta, tb, ycbcr=ycbcr)
        for x, y in zip(first, again):
            assert torch.equal(x.view(torch.int64), y.view(torch.int64))
        for i in range(5):
            alone = metrics.psnr_ssim(ta[i:i + 1], tb[i:i + 1], ycbcr=ycbcr)
            for x, y in zip(first, alone):
                assert x.view(torch.int64)[i].item() == y.view(torch.int64)[0].item(), (ycbcr, i)


# ---- 7. bad arguments through the raw C ABI ---------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments():
    lib = _native.load()
    a = torch.zeros(1, 3, 32, 32, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(64, dtype=torch.int64, device="cuda")
    sse, cnt = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    ssim = torch.zeros(1, dtype=torch.float64, device="cuda")
    taps = (ctypes.c_double * 11)(*metrics.gauss_taps())
    s = _native.stream_handle()

    def call(pa=a.data_ptr(), pb=a.data_ptr(), n=1, c=3, h=32, w=32, border=0, ycbcr=0, with_ssim=1, win=taps, pws=ws.data_ptr(),
             psse=sse.data_ptr(), pcnt=cnt.data_ptr(), pssim=ssim.data_ptr()):
        return lib.virnet_psnr_ssim(pa, 0, pb, 0, n, c, h, w, border, ycbcr, with_ssim, win, pws, psse, pcnt, pssim, s)

    assert call() == 0
    for bad in (dict(pa=0), dict(pb=0), dict(pws=0), dict(psse=0), dict(pcnt=0), dict(pssim=0), dict(win=None), dict(h=10), dict(w=10),
                dict(border=-1), dict(border=11), dict(c=2), dict(c=4), dict(c=1, ycbcr=1), dict(n=0), dict(h=0, with_ssim=0)):
        assert call(**bad) != 0, bad
        assert lib.virnet_last_error(), bad
    assert call(border=11, with_ssim=0) == 0                 # 10 x 10 is enough for PSNR alone
    out = torch.zeros(16, dtype=torch.uint8, device="cuda")
    x = torch.zeros(16, device="cuda")
    assert lib.virnet_quantize_u8(0, out.data_ptr(), 16, s) != 0 and lib.virnet_quantize_u8(x.data_ptr(), 0, 16, s) != 0
    assert lib.virnet_quantize_u8(x.data_ptr(), out.data_ptr(), 0, s) != 0
    assert lib.virnet_rgb2y_u8(0, out.data_ptr(), 1, 2, 2, s) != 0 and lib.virnet_rgb2y_u8(a.data_ptr(), 0, 1, 2, 2, s) != 0
    assert lib.virnet_rgb2y_u8(a.data_ptr(), out.data_ptr(), 1, 0, 2, s) != 0
    torch.cuda.synchronize()


# ---- 8. tables -------------------------------------------------------------------------------------------------------------------------
def _subset(tmp_path, folder, ext, count):
    dst = tmp_path / folder
    dst.mkdir()
    files = sorted(glob.glob(os.path.join(GOLDEN, folder, "*." + ext)))[:count]
    for f in files:
        shutil.copy(f, dst / os.path.basename(f))
    return f"{dst}:{ext}", files


def _synth(net, **kw):
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, **kw), strict=True)
    return net.cuda().eval()


def _compare_rows(host_rows, dev_rows, per_image_key, ssim_key, recompute):
    """``recompute(row index)`` -> (per-image PSNR, mean SSIM) of the host metric on the device's Y planes, for rows that hit a tie."""
    assert len(host_rows) == len(dev_rows) > 0
    for i, (hr, dr) in enumerate(zip(host_rows, dev_rows)):
        assert list(hr) == list(dr) and all(type(hr[k]) is type(dr[k]) for k in hr)
        want_psnr, want_ssim = hr[per_image_key], hr[ssim_key]
        if dr[per_image_key] != want_psnr and recompute is not None:
            print(f"row {i}: a Y plane hits a tie pixel; comparing through the device's planes")
            want_psnr, want_ssim = recompute(i)
        assert dr[per_image_key] == want_psnr, (i, dr[per_image_key], want_psnr)
        assert abs(dr[ssim_key] - want_ssim) <= SSIM_TOL, (i, dr[ssim_key], want_ssim)
        for k in hr:
            if k not in (per_image_key, ssim_key, "psnr", "psnr_y"):
                assert hr[k] == dr[k]
        assert dr[per_image_key.replace("per_image_", "")] == float(np.mean(dr[per_image_key]))


def test_denoise_table_device_metrics_matches_host(tmp_path):
    from virnet_amd.networks import VIRAttResUNet
    spec, _ = _subset(tmp_path, "cbsd68", "png", 4)
    net = _synth(VIRAttResUNet(im_chn=3, sigma_chn=1, n_feat=[96, 192, 288], dep_S=5, n_resblocks=3, noise_cond=True, extra_mode="Input",
                               noise_avg=False))

    def run(noisy):
        with torch.no_grad():
            return net(torch.from_numpy(np.ascontiguousarray(noisy.transpose(2, 0, 1)[np.newaxis])).cuda())[0]

    host = veval.denoise_table(lambda noisy: hwc(run(noisy)[0]), [spec], noise_type="iid", device_metrics=False)
    dev = veval.denoise_table(run, [spec], noise_type="iid", device_metrics=True)
    assert [r["case"] for r in dev] == [15, 25, 50] and all(r["images"] == 4 for r in dev)
    _compare_rows(host, dev, "per_image_psnr", "ssim", None)
    dev3 = veval.denoise_table(lambda noisy: run(noisy)[0], [spec], noise_type="iid", device_metrics=True, with_ssim=False)   # [3,H,W]
    assert [r["per_image_psnr"] for r in dev3] == [r["per_image_psnr"] for r in dev] and all(np.isnan(r["ssim"]) for r in dev3)


def test_sisr_table_device_metrics_matches_host(tmp_path):
    from virnet_amd.networks import VIRAttResUNetSR
    sf = 4
    spec, files = _subset(tmp_path, "set5", "bmp", 2)
    kernels = sisr_eval.test_kernels(sf)[:2]
    net = _synth(VIRAttResUNetSR(im_chn=3, sigma_chn=1, kernel_chn=3, n_feat=[96, 160, 224], dep_S=5, dep_K=8, noise_cond=True,
                                 kernel_cond=True, n_resblocks=2, extra_mode="Both", noise_avg=True))

    def run(lr, sf_):
        with torch.no_grad():
            return net(torch.from_numpy(np.ascontiguousarray(lr.transpose(2, 0, 1)[np.newaxis])).cuda(), sf_)[0]

    host = sisr_eval.sisr_table(lambda lr, s: hwc(run(lr, s)[0]), [spec], sf, kernels=kernels, device_metrics=False)
    dev = sisr_eval.sisr_table(run, [spec], sf, kernels=kernels, device_metrics=True)

    def recompute(i):
        psnrs, ssims = [], []
        for f in files:
            gt = sisr_eval.modcrop(veval.imread_rgb_uint8(f), sf)
            sr = veval.img_as_ubyte(np.clip(hwc(run(sisr_eval.degrade(veval.img_as_float32(gt), kernels[i], sf), sf)[0]), 0.0, 1.0))
            _, _, p, q = host_numbers(sr, gt, sf ** 2, True)
            psnrs.append(p)
            ssims.append(q)
        return psnrs, float(np.mean(ssims))

    assert [r["kernel"] for r in dev] == [1, 2] and all(r["images"] == 2 for r in dev)
    _compare_rows(host, dev, "per_image_psnr_y", "ssim_y", recompute)


# ---- 9. non-current device -------------------------------------------------------------------------------------------------------------
def test_inputs_on_a_non_current_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    a, b = pair(97, 131, seed=77)
    ta, tb = nchw(a)[None], nchw(b)[None]
    here = metrics.psnr_ssim(ta.cuda(0), tb.cuda(0), border=2)
    with torch.cuda.device(0):
        there = metrics.psnr_ssim(ta.to("cuda:1"), tb.to("cuda:1"), border=2)
        y1 = metrics.rgb2y(ta.to("cuda:1"))
        q1 = metrics.to_uint8((ta.float() / 255.0).to("cuda:1"))
    assert all(t.device == torch.device("cuda:1") for t in there) and y1.device == q1.device == torch.device("cuda:1")
    for x, y in zip(here, there):
        assert torch.equal(x.view(torch.int64).cpu(), y.view(torch.int64).cpu())
    assert torch.equal(q1.cpu(), ta) and np.array_equal(y1[0, 0].cpu().numpy(), metrics.rgb2y(ta.cuda(0))[0, 0].cpu().numpy())
