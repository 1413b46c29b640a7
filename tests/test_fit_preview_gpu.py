"""The summary-writer hook of the training loops (``writer=`` of ``fit.fit_denoising`` / ``fit.fit_sisr``; virnet_amd/preview.py) at the tiny
networks of tests/test_fit_gpu.py and tests/test_fit_sisr_gpu.py with ``print_freq=1``: the exact sequence of writer calls, the event
counters in the returned dictionary and the checkpoints, a resume that continues them, ONE ``to_host`` per event -- and the run itself
bit for bit the run without a writer, which never enters the preview module."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from virnet_amd import datagen, fit
from virnet_amd import eval as veval
from virnet_amd import preview as pv
from virnet_amd.networks import VIRAttResUNet, VIRAttResUNetSR
from virnet_amd.utils.synth import synth_state_dict

pytestmark = pytest.mark.gpu

NET = dict(sigma_chn=1, n_feat=[32, 64], dep_S=3, n_resblocks=1)
CFG = dict(batch_size=4, patch_size=32, epochs=2, warmup_epochs=1, lr=1e-4, lr_min=1e-6, print_freq=1, clip_grad_R=1e3, clip_grad_S=1e2,
           var_window=7, eps2=1e-6, steps_per_epoch=50)
SMALL = dict(im_chn=3, sigma_chn=1, kernel_chn=3, n_feat=[64, 96], dep_S=3, dep_K=2, noise_cond=True, kernel_cond=True, n_resblocks=1,
             extra_mode="Both", noise_avg=True)
SISR_CFG = dict(im_chn=3, sigma_chn=1, hr_size=48, batch_size=4, epochs=2, lr=2e-4, lr_min=1e-6, print_freq=1, sf=2, k_size=21, add_jpeg="False",
                kernel_shift="False", downsampler="Bicubic", noise_level=[0.01, 15], noise_jpeg=[0.01, 10], eps2=1e-5, r2=1e-4, var_window=9,
                kappa0=50, penalty_K=[0.02, 2], clip_grad_R=5e2, clip_grad_S=1e2, clip_grad_K=5e2, steps_per_epoch=20)
OUT_KEYS = {"epoch_start", "lr", "train", "psnr", "ssim", "val_images", "checkpoints", "optimizer", "rows", "step", "step_img", "world", "rank"}
CKPT_KEYS = {"epoch", "step", "step_img", "model_state_dict", "optimizer_state_dict"}
ENTRY_POINTS = ("grid", "grids", "kernel_from_kinfo", "to_host", "denoise_train", "denoise_test", "sisr_train", "sisr_test")


class Recorder:
    """A writer that records its calls: (method, tag, step) and what came with them."""

    def __init__(self):
        self.calls, self.values = [], []

    def add_scalar(self, tag, value, step):
        assert type(value) is float and type(step) is int
        self.calls.append(("add_scalar", tag, step))
        self.values.append(value)

    def add_image(self, tag, image, step, dataformats="CHW"):
        assert dataformats == "HWC" and isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
        assert type(step) is int
        self.calls.append(("add_image", tag, step))
        self.values.append(image.copy())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_state(sd_a, sd_b):
    return list(sd_a) == list(sd_b) and all(_same(sd_a[k], sd_b[k]) for k in sd_a)


def _same_adam(sa, sb):
    sa, sb = sa["state"], sb["state"]
    return sa.keys() == sb.keys() and len(sa) > 0 and all(
        float(sa[k]["step"]) == float(sb[k]["step"]) and _same(sa[k]["exp_avg"], sb[k]["exp_avg"]) and _same(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"])
        for k in sa)


def _zeroed(net):
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()                                                              # (everything must come from the checkpoint)
    return net


def _counted(monkeypatch_ctx):
    """``preview.to_host`` replaced by a wrapper that counts its calls"""
    count, orig = [0], pv.to_host

    def to_host(grids):
        count[0] += 1
        return orig(grids)
    monkeypatch_ctx.setattr(pv, "to_host", to_host)
    return count


def _forbid(monkeypatch_ctx):
    def refuse(*a, **k):
        raise AssertionError("a run without a writer entered the preview module")
    for name in ENTRY_POINTS:
        monkeypatch_ctx.setattr(pv, name, refuse)


def _train_calls(epoch, num_iter, first_step, train_tags, n_train_before):
    """the calls of one epoch's training part at print_freq 1 with one preview event, at the epoch's last step"""
    calls = [("add_scalar", "Train Loss Iter", first_step + ii) for ii in range(num_iter)]
    calls += [("add_image", tag, n_train_before) for tag in train_tags]
    return calls + [("add_scalar", "Loss_epoch", epoch)]


# ---- denoising ---------------------------------------------------------------------------------------------------------------------------------
TRAIN_TAGS = ["train Denoised images", "train GroundTruth", "train Predict Sigma", "train Groundtruth Sigma", "train Noisy Image"]
TEST_TAGS = ["test Denoised images", "test GroundTruth", "test Predict Sigma", "test Noise Image"]


def _net():
    net = VIRAttResUNet(3, **NET)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=11))
    return net.cuda()


@pytest.fixture(scope="module")
def data():
    g = np.random.default_rng(1)
    pool = datagen.ImagePool([g.integers(0, 256, (48, 48, 3), dtype=np.uint8) for _ in range(4)], "cuda")
    shapes = [(24, 20), (20, 24)] * 10 + [(24, 20)]                                 # 21 images in two shape groups: the 20th gets the event
    val = datagen.SimulateTestSet(datagen.ImagePool([g.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes], "cuda"))
    return pool, val


@pytest.fixture(scope="module")
def plain_run(data, tmp_path_factory):
    """without a writer -- and with every entry point of the preview module replaced by one that raises"""
    net = _net()
    with pytest.MonkeyPatch.context() as mp:
        _forbid(mp)
        out = fit.fit_denoising(net, data[0], CFG, val=data[1], save_dir=tmp_path_factory.mktemp("plain"), log=lambda s: None)
    return dict(net=net, out=out)


@pytest.fixture(scope="module")
def writer_run(data, tmp_path_factory):
    net, rec = _net(), Recorder()
    with pytest.MonkeyPatch.context() as mp:
        count = _counted(mp)
        out = fit.fit_denoising(net, data[0], CFG, val=data[1], save_dir=tmp_path_factory.mktemp("writer"), log=lambda s: None, writer=rec)
    return dict(net=net, out=out, rec=rec, to_host_calls=count[0])


def _denoise_epoch_calls(epoch, first_step, events_before):
    return (_train_calls(epoch, 50, first_step, TRAIN_TAGS, events_before) + [("add_image", tag, events_before) for tag in TEST_TAGS]
            + [("add_scalar", "PSNR_epoch_test", epoch), ("add_scalar", "SSIM_epoch_test", epoch)])


def test_the_writer_receives_the_references_calls(writer_run, data):
    rec, out = writer_run["rec"], writer_run["out"]
    assert rec.calls == _denoise_epoch_calls(0, 0, 0) + _denoise_epoch_calls(1, 50, 1)
    assert writer_run["to_host_calls"] == 4                                         # one per event: two train events, two test events
    by_call = dict(zip(rec.calls, rec.values))
    # the scalars are the loop's own numbers
    assert [by_call[("add_scalar", "Train Loss Iter", s)] for s in range(100)] == [float(v) for v in out["rows"][:, 0]]
    assert [by_call[("add_scalar", "Loss_epoch", e)] for e in range(2)] == [t["Loss"] for t in out["train"]]
    assert [by_call[("add_scalar", "PSNR_epoch_test", e)] for e in range(2)] == out["psnr"]
    assert [by_call[("add_scalar", "SSIM_epoch_test", e)] for e in range(2)] == out["ssim"]
    # shapes: a train grid holds the batch of four 32 x 32 patches, a test grid is the bare 20th image (index 19: 20 x 24)
    for e in range(2):
        for tag in TRAIN_TAGS:
            assert by_call[("add_image", tag, e)].shape == (36, 4 * 34 + 2, 3)
        for tag in TEST_TAGS:
            assert by_call[("add_image", tag, e)].shape == (20, 24, 3)
        # the ground truth of the test event is the validation set's own image, normalised
        _, im_gt = data[1].batch([19])
        assert np.array_equal(by_call[("add_image", "test GroundTruth", e)], pv.grid_np(im_gt.cpu().numpy()))
    assert not np.array_equal(by_call[("add_image", "train Denoised images", 0)], by_call[("add_image", "train Denoised images", 1)])


def test_step_img_counts_the_events(writer_run, plain_run):
    assert writer_run["out"]["step_img"] == {"train": 2, "test": 2} and plain_run["out"]["step_img"] == {"train": 0, "test": 0}
    assert set(writer_run["out"]) == OUT_KEYS and set(plain_run["out"]) == OUT_KEYS
    for k in range(2):
        with_w = torch.load(writer_run["out"]["checkpoints"][k], map_location="cpu")
        without = torch.load(plain_run["out"]["checkpoints"][k], map_location="cpu")
        assert set(with_w) == CKPT_KEYS and set(without) == CKPT_KEYS
        assert with_w["step_img"] == {"train": k + 1, "test": k + 1} and without["step_img"] == {"train": 0, "test": 0}


def test_the_run_is_bitwise_the_run_without_a_writer(writer_run, plain_run):
    a, b = plain_run["out"], writer_run["out"]
    assert _same_state(plain_run["net"].state_dict(), writer_run["net"].state_dict())
    assert a["rows"].shape == (100, 6) and np.array_equal(a["rows"].view(np.uint32), b["rows"].view(np.uint32))
    assert a["train"] == b["train"] and a["lr"] == b["lr"] and a["psnr"] == b["psnr"] and a["ssim"] == b["ssim"] and a["step"] == b["step"] == 100
    for k in range(2):
        ca, cb = (torch.load(o["checkpoints"][k], map_location="cpu") for o in (a, b))
        assert _same_state(ca["model_state_dict"], cb["model_state_dict"]) and _same_adam(ca["optimizer_state_dict"], cb["optimizer_state_dict"])
        assert ca["epoch"] == cb["epoch"] and ca["step"] == cb["step"]


def test_a_resume_continues_the_counters(writer_run, data, tmp_path):
    first = writer_run["out"]["checkpoints"][0]
    ckpt = torch.load(first, map_location="cpu")
    net, rec = _zeroed(_net()), Recorder()
    out = fit.fit_denoising(net, data[0], CFG, val=data[1], save_dir=tmp_path, log=lambda s: None, writer=rec, resume=first)
    assert rec.calls == _denoise_epoch_calls(1, ckpt["step"], 1)                    # (the reference's checkpoint stores step + 1)
    assert out["step_img"] == {"train": 2, "test": 2} and torch.load(out["checkpoints"][0], map_location="cpu")["step_img"] == {"train": 2, "test": 2}
    assert _same_state(net.state_dict(), writer_run["net"].state_dict())
    images = [v for c, v in zip(rec.calls, rec.values) if c[0] == "add_image"]
    want = [v for c, v in zip(writer_run["rec"].calls, writer_run["rec"].values) if c[0] == "add_image" and c[2] == 1]
    assert len(images) == 9 and all(np.array_equal(x, y) for x, y in zip(images, want))


def test_without_val_the_test_scalars_are_skipped(data, tmp_path):
    rec = Recorder()
    cfg = dict(CFG, epochs=2, steps_per_epoch=2, print_freq=2)
    out = fit.fit_denoising(_net(), data[0], cfg, save_dir=tmp_path, log=lambda s: None, writer=rec)
    # print_freq 2: the first and the second step are printed; no step is a multiple of 50 * 2, so no image
    want = []
    for e in range(2):
        want += [("add_scalar", "Train Loss Iter", 2 * e), ("add_scalar", "Train Loss Iter", 2 * e + 1), ("add_scalar", "Loss_epoch", e)]
    assert rec.calls == want and out["step_img"] == {"train": 0, "test": 0}


# ---- SISR --------------------------------------------------------------------------------------------------------------------------------------
SISR_TRAIN_TAGS = ["train Recover Image", "train HR Image", "train GT Blur Kernel", "train LR Image", "train Est Blur Kernel Resample",
                   "train Est Blur Kernel"]
SISR_TEST_TAGS = ["Test Gaussian Recover images", "Test Gaussian HR Image", "Test Gaussian LR Image", "Test Gaussian GT Blur Kernel",
                  "Test Gaussian Est Blur Kernel"]


def _sisr_net():
    net = VIRAttResUNetSR(**SMALL)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=5), strict=True)
    return net.cuda()


@pytest.fixture(scope="module")
def sisr_data():
    files = sorted(glob.glob(os.path.join(GOLDEN, "cbsd68", "*.png")))[:4]
    pool = datagen.ImagePool([veval.imread_rgb_uint8(f) for f in files], "cuda")
    g = load_golden("general_test")
    crops = [g["u8_0"], g["u8_1"], np.ascontiguousarray(g["u8_0"][::-1])]           # three images: the third gets the event
    return pool, datagen.GeneralTestSet(datagen.ImagePool(crops, "cuda"), 2)


@pytest.fixture(scope="module")
def sisr_plain_run(sisr_data, tmp_path_factory):
    net = _sisr_net()
    with pytest.MonkeyPatch.context() as mp:
        _forbid(mp)
        out = fit.fit_sisr(net, sisr_data[0], SISR_CFG, val=sisr_data[1], save_dir=tmp_path_factory.mktemp("sisr_plain"), log=lambda s: None)
    return dict(net=net, out=out)


@pytest.fixture(scope="module")
def sisr_writer_run(sisr_data, tmp_path_factory):
    net, rec = _sisr_net(), Recorder()
    with pytest.MonkeyPatch.context() as mp:
        count = _counted(mp)
        out = fit.fit_sisr(net, sisr_data[0], SISR_CFG, val=sisr_data[1], save_dir=tmp_path_factory.mktemp("sisr_writer"), log=lambda s: None, writer=rec)
    return dict(net=net, out=out, rec=rec, to_host_calls=count[0])


def _sisr_epoch_calls(epoch, first_step, events_before):
    return (_train_calls(epoch, 20, first_step, SISR_TRAIN_TAGS, events_before) + [("add_image", tag, events_before) for tag in SISR_TEST_TAGS]
            + [("add_scalar", "Gaussian PSNR Test", epoch), ("add_scalar", "Gaussian SSIM Test", epoch)])


def test_sisr_writer_calls_counters_and_bitwise_run(sisr_writer_run, sisr_plain_run, sisr_data):
    rec, out, plain = sisr_writer_run["rec"], sisr_writer_run["out"], sisr_plain_run["out"]
    assert rec.calls == _sisr_epoch_calls(0, 0, 0) + _sisr_epoch_calls(1, 20, 1)
    assert sisr_writer_run["to_host_calls"] == 4
    by_call = dict(zip(rec.calls, rec.values))
    assert [by_call[("add_scalar", "Train Loss Iter", s)] for s in range(40)] == [float(v) for v in out["rows"][:, 0]]
    assert [by_call[("add_scalar", "Gaussian PSNR Test", e)] for e in range(2)] == out["psnr"]["Gaussian"]
    assert [by_call[("add_scalar", "Gaussian SSIM Test", e)] for e in range(2)] == out["ssim"]["Gaussian"]
    im_hr, im_lr, kinfo = sisr_data[1].batch([2])
    for e in range(2):
        assert by_call[("add_image", "train HR Image", e)].shape == (52, 4 * 50 + 2, 3)
        assert by_call[("add_image", "train GT Blur Kernel", e)].shape == by_call[("add_image", "train Est Blur Kernel", e)].shape == (25, 4 * 23 + 2, 3)
        assert by_call[("add_image", "Test Gaussian Recover images", e)].shape == tuple(im_hr.shape[2:]) + (3,)
        assert np.array_equal(by_call[("add_image", "Test Gaussian HR Image", e)], pv.grid_np(im_hr.cpu().numpy()))
        assert np.array_equal(by_call[("add_image", "Test Gaussian LR Image", e)], pv.grid_np(im_lr.cpu().numpy()))
        assert np.array_equal(by_call[("add_image", "Test Gaussian GT Blur Kernel", e)], pv.grid_np(pv.kernel_from_kinfo(kinfo, 21, 2, False).cpu().numpy()))
    # counters, here and in the checkpoints
    assert out["step_img"] == {"train": 2, "Gaussian": 2} and plain["step_img"] == {"train": 0, "Gaussian": 0}
    assert set(out) == OUT_KEYS and set(plain) == OUT_KEYS
    for k in range(2):
        ca, cb = (torch.load(o["checkpoints"][k], map_location="cpu") for o in (plain, out))
        assert set(ca) == CKPT_KEYS and set(cb) == CKPT_KEYS
        assert ca["step_img"] == {"train": 0, "Gaussian": 0} and cb["step_img"] == {"train": k + 1, "Gaussian": k + 1}
        assert _same_state(ca["model_state_dict"], cb["model_state_dict"]) and _same_adam(ca["optimizer_state_dict"], cb["optimizer_state_dict"])
    # the run itself: bit for bit the run without a writer (the previews draw from no generator)
    assert _same_state(sisr_plain_run["net"].state_dict(), sisr_writer_run["net"].state_dict())
    assert plain["rows"].shape == (40, 8) and np.array_equal(plain["rows"].view(np.uint32), out["rows"].view(np.uint32))
    assert plain["psnr"] == out["psnr"] and plain["ssim"] == out["ssim"] and plain["train"] == out["train"]


def test_sisr_resume_continues_the_counters(sisr_writer_run, sisr_data, tmp_path):
    first = sisr_writer_run["out"]["checkpoints"][0]
    ckpt = torch.load(first, map_location="cpu")
    net, rec = _zeroed(_sisr_net()), Recorder()
    out = fit.fit_sisr(net, sisr_data[0], SISR_CFG, val=sisr_data[1], save_dir=tmp_path, log=lambda s: None, writer=rec, resume=first)
    assert rec.calls == _sisr_epoch_calls(1, ckpt["step"], 1)
    assert out["step_img"] == {"train": 2, "Gaussian": 2}
    assert _same_state(net.state_dict(), sisr_writer_run["net"].state_dict())
