"""Host side of the SISR training loop (virnet_amd/fit.py fit_sisr, schedule.cosine, metrics.rgb2y_float_np, datagen.general_test_np /
general_noise, the bindings of the order-fixed SFT backward and of the float-Y metric mode): the definitions against the installed torch
and against what the reference's own ``GeneralTest`` returned (tests/golden/general_test.npz), the config reader on the reference's three
SISR configs (tests/golden/configs, copied unchanged), the log lines against the reference's format strings, and the C entries'
refusals, which fire before any launch.  No GPU is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, load_golden
from virnet_amd import _native, datagen, fit, metrics, schedule
from virnet_amd import eval as veval

CONFIGS = os.path.join(GOLDEN, "configs")


# ---- schedule --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr,lr_min,epochs", [(2e-4, 1e-6, 120), (1e-4, 0, 3)])
def test_cosine_is_torchs_list_double_for_double(lr, lr_min, epochs):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer=opt, T_max=epochs, eta_min=lr_min)          # train_SISR.py:98-101
    want = []
    for _ in range(epochs):
        want.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()                                                                                       # :324
    got = schedule.cosine(lr, lr_min, epochs)
    assert got == want and all(isinstance(v, float) for v in got)
    closed = [lr_min + (lr - lr_min) * (1 + np.cos(np.pi * e / epochs)) / 2 for e in range(epochs)]
    print("entries that differ from the closed form:", sum(a != b for a, b in zip(got, closed)), "of", epochs)
    assert max(abs(a - b) for a, b in zip(got, closed)) <= 1e-15
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            schedule.cosine(lr, lr_min, bad)


# ---- config ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sf,hr,clip", [("sisr_x2", 2, 96, (1e2, 1e2, 1e2)), ("sisr_x3", 3, 144, (5e2, 1e2, 5e2)), ("sisr_x4", 4, 192, (5e2, 1e2, 5e2))])
def test_read_sisr_config_on_the_reference_configs(name, sf, hr, clip):
    raw = fit.load_config(os.path.join(CONFIGS, name + ".json"))
    assert raw["add_jpeg"] == "False" and raw["noise_cond"] == "True"                  # the booleans are strings (util_opts.str2bool)
    c = fit.read_sisr_config(raw)
    assert (c["sf"], c["hr_size"], c["batch_size"], c["epochs"], c["k_size"], c["var_window"]) == (sf, hr, 16, 120, 21, 9)
    assert (c["clip_grad_R"], c["clip_grad_S"], c["clip_grad_K"]) == clip
    assert c["add_jpeg"] is False and c["kernel_shift"] is False and c["downsampler"] == "Bicubic"
    assert c["noise_level"] == [0.01, 15.0] and c["noise_jpeg"] == [0.01, 10.0] and c["penalty_K"] == [0.02, 2.0]
    assert c["steps_per_epoch"] == 10000 and c["print_freq"] == 100 and c["kappa0"] == 50.0 and c["r2"] == 1e-4 and c["eps2"] == 1e-5
    assert all(isinstance(c[k], int) for k in ("sf", "hr_size", "batch_size", "epochs", "k_size", "var_window", "steps_per_epoch"))


def test_read_sisr_config_refusals():
    raw = fit.load_config(os.path.join(CONFIGS, "sisr_x4.json"))
    with pytest.raises(TypeError):
        fit.read_sisr_config([("sf", 4)])
    with pytest.raises(KeyError, match="clip_grad_K"):
        fit.read_sisr_config({k: v for k, v in raw.items() if k != "clip_grad_K"})
    for key, bad, what in (("add_jpeg", "yes", "'True' or 'False'"), ("kernel_shift", 1, "'True' or 'False'"), ("sf", 2.5, "positive integer"),
                           ("sf", "4", "positive integer"), ("batch_size", 0, "positive integer"), ("lr", -1e-4, "non-negative"),
                           ("clip_grad_K", "5e2", "non-negative"), ("noise_level", [15, 0.1], "increasing"), ("noise_jpeg", [1], "two numbers"),
                           ("penalty_K", 0.02, "two numbers"), ("downsampler", "nearest", "Direct"), ("hr_size", 190, "multiple of sf"),
                           ("kappa0", 1, "kappa0 > 1")):
        with pytest.raises(ValueError, match=what):
            fit.read_sisr_config(dict(raw, **{key: bad}))
    assert fit.read_sisr_config(dict(raw, add_jpeg="TRUE", kernel_shift=True, steps_per_epoch=7))["add_jpeg"] is True


def test_fit_sisr_checks_noise_avg_before_any_device_work():
    """train_SISR.py:87 builds the net with noise_avg = not add_jpeg; a mismatch is a ValueError (raised before the pool is looked at)."""
    raw = fit.load_config(os.path.join(CONFIGS, "sisr_x2.json"))

    class Net(torch.nn.Module):
        noise_avg = False

    pool = datagen.ImagePool([np.zeros((96, 96, 3), dtype=np.uint8)], "cpu")
    with pytest.raises(ValueError, match="noise_avg=True"):
        fit.fit_sisr(Net(), pool, raw)
    net = Net()
    net.noise_avg = True
    with pytest.raises(ValueError, match="noise_avg=False"):
        fit.fit_sisr(net, pool, dict(raw, add_jpeg="True"))
    with pytest.raises(RuntimeError, match="ROCm device only"):                          # the check passed: the CPU pool is refused next
        fit.fit_sisr(net, pool, raw)


# ---- lines -----------------------------------------------------------------------------------------------------------------------------------
def test_lines_are_the_references_character_for_character():
    """The reference's format strings (train_SISR.py:239-243, 267-269, 291-293, 319-320), restated."""
    row = np.asarray([-1234.5678, 3.14159, -0.5, 12345.678, 0.001, 1234.5, 0.0123, 5e5], dtype=np.float32)
    log_str = '[Epoch:{:>3d}/{:<3d}] {:s}:{:0>5d}/{:0>5d}, lh:{:+>5.2f}, KL:{:+>7.2f}/{:+>6.2f}/{:+>6.2f}, ' + \
              'Grad:{:.1e}/{:.1e}/{:.1e}, lr={:.1e}'
    for epoch, ii, lr in ((0, 0, 2e-4), (119, 9999, 1.0340961649320526e-06), (9, 99, 1.5e-4)):
        want = log_str.format(epoch + 1, 120, "train", ii + 1, 10000, torch.tensor(row[1]).item(), torch.tensor(row[2]).item(),
                              torch.tensor(row[3]).item(), torch.tensor(row[4]).item(), torch.tensor(row[5]), torch.tensor(row[6]),
                              torch.tensor(row[7]), lr)
        assert fit.sisr_train_line(epoch, 120, ii, 10000, row, lr) == want
    assert fit.sisr_train_line(0, 120, 0, 10000, row, 2e-4).startswith("[Epoch:  1/120] train:00001/10000, lh:+3.14, KL:++-0.50/12345.68/++0.00, Grad:1.2e+03/")
    sums = [-1.2345e3, 3.14159, -0.5, 123.456, 0.001]
    log_str = '{:s}: Loss={:+.2e}, lh={:>4.2f}, KLR={:+>7.2f}, KLS={:+>6.2f}, KLK={:+>5.2f}'
    assert fit.sisr_epoch_line(sums) == log_str.format("train", *sums)
    log_str = 'Noise: {:s}, Epoch:{:>3d}/{:<3d}] {:s}:{:0>3d}/{:0>3d}, psnr={:4.2f}, ssim={:5.4f}'
    assert fit.sisr_test_line("JPEG", 4, 120, 2, 14, 27.123456, 0.812345) == log_str.format("JPEG", 5, 120, "test", 3, 14, 27.123456, 0.812345)
    log_str = 'Noise: {:s}, {:s}: PSNR={:4.2f}, SSIM={:5.4f}'
    assert fit.sisr_summary_line("Gaussian", 9.5, 0.5) == log_str.format("Gaussian", "test", 9.5, 0.5)


# ---- the float-Y definition ------------------------------------------------------------------------------------------------------------------
def _rgb2ycbcr_torch(im):
    """util_image.rgb2ycbcrTorch(im, only_y=True) (:155-176), restated."""
    im_temp = im.permute([0, 2, 3, 1]) * 255.0
    rlt = torch.matmul(im_temp, torch.tensor([65.481, 128.553, 24.966], device=im.device, dtype=im.dtype).view([3, 1]) / 255.0) + 16.0
    rlt /= 255.0
    rlt.clamp_(0.0, 1.0)
    return rlt.permute([0, 3, 1, 2])


def float_y_inputs():
    torch.manual_seed(0)
    a = torch.rand(4, 3, 96, 128)
    b = torch.rand(4, 3, 96, 128) * 1.4 - 0.2
    c = torch.randint(0, 256, (4, 3, 96, 128), dtype=torch.uint8).float() / 255
    return a, b, c


def test_rgb2y_float_np_against_the_torch_expression():
    for name, im in zip(("unit", "beyond [0,1]", "bytes / 255"), float_y_inputs()):
        got, want = metrics.rgb2y_float_np(im.numpy()), _rgb2ycbcr_torch(im).numpy()
        assert got.shape == want.shape == (4, 1, 96, 128) and got.dtype == np.float32
        share = float((got.view(np.uint32) != want.view(np.uint32)).mean())
        print(f"{name}: share of floats that differ from torch's matmul expression: {share}")
        assert np.array_equal(veval.img_as_ubyte(got), veval.img_as_ubyte(want))          # the bytes the metric compares: identical everywhere
    with pytest.raises(ValueError):
        metrics.rgb2y_float_np(np.zeros((1, 1, 4, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        metrics.rgb2y_float_np(np.zeros((1, 3, 4, 4), dtype=np.float64))


def test_psnr_ssim_float_mode_argument_checks():
    a = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match="'float'"):
        metrics.psnr_ssim(a, a, ycbcr="y")
    with pytest.raises(TypeError, match="float32 images"):
        metrics.psnr_ssim(a.to(torch.uint8), a, ycbcr="float")
    with pytest.raises(ValueError, match="RGB"):
        metrics.psnr_ssim(a[:, :1], a[:, :1], ycbcr="float")
    with pytest.raises(RuntimeError, match="ROCm device only"):                          # the checks passed: CPU tensors are refused next
        metrics.psnr_ssim(a, a, ycbcr="float")


# ---- the validation set's definition -----------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return int(np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64)).max())


@pytest.mark.parametrize("case", ["sf2", "sf4", "sf2s"])
def test_general_test_np_is_what_the_reference_returned(case):
    g = load_golden("general_test")
    images = [g["u8_0"], g["u8_1"]]
    assert [im.shape for im in images] == [(44, 60, 3), (60, 44, 3)]
    sf, down, seed, shift = int(g[case + "_sf"]), str(g[case + "_downsampler"]), int(g["seed"]), bool(g[case + "_shift"])
    assert shift == (case == "sf2s")          # (the half-pixel centre: an asymmetric kernel, so the direction of the convolution shows)
    noise = datagen.general_noise([im.shape[:2] for im in images], sf, seed)
    want_noise = g[case + "_noise"]
    assert noise.shape == want_noise.shape == (60 // sf, 60 // sf, 3) and noise.dtype == np.float32
    assert np.array_equal(noise.view(np.uint32), want_noise.view(np.uint32))
    got = datagen.general_test_np(images, sf, 21, shift, down, "Gaussian", seed=seed)
    for i, (im_hr, im_lr, kinfo) in enumerate(got):
        want_hr, want_lr, want_k = g[f"{case}_hr_{i}"], g[f"{case}_lr_{i}"], g[f"{case}_kinfo_{i}"]
        assert im_hr.dtype == im_lr.dtype == kinfo.dtype == np.float32 and im_lr.shape == want_lr.shape
        assert im_hr.shape == want_hr.shape and np.array_equal(im_hr.view(np.uint32), want_hr.view(np.uint32))
        err = float(np.abs(im_lr - want_lr).max())
        print(case, i, "im_lr max |error|", err, "kinfo ulps", _ulps(kinfo, want_k))
        assert _ulps(kinfo, want_k) <= 1
        assert err <= 1e-6          # (the bar tests/test_datagen_host.py holds sisr_batch_np to)


def test_general_test_np_jpeg_and_refusals():
    """The JPEG variant has no reference golden (tests/golden/make_general_test_golden.py says why): it is the Gaussian variant pushed
    through ``sisr_eval.synthesize_tail_np``'s quality-40 round trip, whose codec tests/golden/jpeg.npz pins."""
    from virnet_amd import sisr_eval
    g = load_golden("general_test")
    images = [g["u8_0"], g["u8_1"]]
    gauss = datagen.general_test_np(images, 2, 21, False, "direct", "Gaussian")
    jpeg = datagen.general_test_np(images, 2, 21, False, "direct", "JPEG")
    for (hr_a, lr_a, k_a), (hr_b, lr_b, k_b) in zip(gauss, jpeg):
        assert np.array_equal(hr_a, hr_b) and np.array_equal(k_a, k_b) and lr_b.dtype == np.float32 and not np.array_equal(lr_a, lr_b)
        zero = np.zeros(lr_a.shape[1:] + (3,), dtype=np.float32)
        want = sisr_eval.synthesize_tail_np(np.ascontiguousarray(lr_a.transpose(1, 2, 0)), zero, 0.0, qf=40)
        assert np.array_equal(lr_b, want.transpose(2, 0, 1))
    for kw in (dict(sf=0), dict(sf=2, k_size=20), dict(sf=2, downsampler="nearest"), dict(sf=2, noise_type="Poisson")):
        with pytest.raises(ValueError):
            datagen.general_test_np(images, **kw)
    with pytest.raises(ValueError, match="smaller than an LR image"):
        datagen.general_test_np(images, 2, noise=np.zeros((10, 10, 3), dtype=np.float32))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        datagen.GeneralTestSet(datagen.ImagePool(images, "cpu"), 2)


# ---- bindings --------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_bound_and_abi_version_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in ("virnet_sft_backward_scratch_bytes", "virnet_sft_backward_ordered", "virnet_sft_backward"):
        assert name in bound and getattr(lib, name) is not None
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5
    with open(os.path.join(REPO, "include", "virnet_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+VIRNET_ABI_VERSION\s+5\b", header)
    for decl in ("size_t virnet_sft_backward_scratch_bytes(int n, long hw, int c);", "int virnet_sft_backward_ordered("):
        assert decl in header
    assert "AttResUNet.py:54-58" in header[header.index("order-fixed sums") - 200:header.index("order-fixed sums")]


def test_the_c_entries_refuse_bad_arguments_before_any_launch():
    lib = _native.load()
    err = lambda: lib.virnet_last_error().decode()          # noqa: E731
    size = lib.virnet_sft_backward_scratch_bytes
    assert size(2, 35, 96) == 2 * 1 * 2 * 96 * 4 and size(1, 1024, 4) == 32 and size(2, 1056, 160) == 2 * 2 * 2 * 160 * 4
    assert size(3, 2050, 224) == 3 * 3 * 2 * 224 * 4 and size(16, 192 * 192, 96) == 16 * 36 * 2 * 96 * 4
    assert size(1, 10, 6) == 0 and size(1, 10, 1028) == 0 and size(0, 10, 8) == 0 and size(1, 0, 8) == 0
    host = np.zeros(1 << 16, dtype=np.float32)          # (host memory: every call below is refused before it would launch)
    base = host.ctypes.data + (-host.ctypes.data) % 256
    n, hw, c = 2, 40, 8
    tb, vb = n * hw * c * 4, 256
    da, x, res, dx = (base + k * tb for k in range(4))
    mul, add, dmul, dadd = (base + 4 * tb + k * vb for k in range(4))
    part = base + 4 * tb + 4 * vb

    def call(**kw):
        a = dict(da=da, x=x, mul=mul, add=add, res=res, slope=0.2, dx=dx, dmul=dmul, dadd=dadd, part=part, n=n, hw=hw, c=c)
        a.update(kw)
        return lib.virnet_sft_backward_ordered(a["da"], a["x"], a["mul"], a["add"], a["res"], a["slope"], a["dx"], a["dmul"], a["dadd"], a["part"],
                                               a["n"], a["hw"], a["c"], None)

    for name in ("da", "x", "mul", "add", "dx", "dmul", "dadd", "part"):
        assert call(**{name: None}) != 0 and "NULL" in err(), name
    assert call(c=6) != 0 and "bad shape" in err()
    assert call(c=1028) != 0 and "bad shape" in err()
    assert call(n=0) != 0 and "bad shape" in err()
    assert call(hw=0) != 0 and "bad shape" in err()
    assert call(slope=1.5) != 0 and "slope" in err()
    assert call(slope=-0.1) != 0 and "slope" in err()
    assert call(part=part + 4) != 0 and "aligned" in err()
    for name, where in (("da", da), ("x", x), ("res", res), ("dx", dx), ("mul", mul), ("add", add), ("dmul", dmul), ("dadd", dadd)):
        assert call(part=where) != 0 and "overlaps" in err(), name
    assert call(part=dx + tb - 16) != 0 and "overlaps" in err()                           # the scratch's head on the output's tail
    # the float-Y mode of the metric: ycbcr = 2 takes float32 RGB only; other values are refused
    ps = lib.virnet_psnr_ssim
    taps = (C.c_double * 11)(*metrics.gauss_taps())
    margs = lambda af, bf, ch, mode: (base, af, base + 8192, bf, 1, ch, 16, 16, 0, mode, 1, taps, base + 16384, base + 20480, base + 20488, base + 20496, None)  # noqa: E731
    assert ps(*margs(0, 1, 3, 2)) != 0 and "float32 inputs" in err()
    assert ps(*margs(1, 0, 3, 2)) != 0 and "float32 inputs" in err()
    assert ps(*margs(1, 1, 1, 2)) != 0 and "3 channels" in err()
    assert ps(*margs(1, 1, 3, 3)) != 0 and "ycbcr=3" in err()
    assert lib.virnet_psnr_ssim_workspace_bytes(1, 3, 16, 16, 0, 2) == lib.virnet_psnr_ssim_workspace_bytes(1, 3, 16, 16, 0, 1) == 16
