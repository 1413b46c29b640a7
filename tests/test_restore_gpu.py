"""GPU tests of tiled whole-image restoration (virnet_amd/restore.py, csrc/restore.hip): both kernels against their host definitions bit
for bit, the end-to-end calls against ``forward_tiled`` / ``forward_tiled_sisr``, the automatic tile, the demo tool, graph capture and the
range guard.  Inputs and references: tests/restore_cases.py."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import restore_cases as rc
from virnet_amd import engine, ops, restore
from virnet_amd import eval as veval
from virnet_amd.networks import VIRAttResUNet, VIRAttResUNetSR
from virnet_amd.utils.synth import synth_images, synth_state_dict
from virnet_amd.utils.tiling import forward_tiled, forward_tiled_sisr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEN_CFG = dict(im_chn=3, sigma_chn=1, n_feat=[96, 192, 288], dep_S=5, n_resblocks=3, noise_cond=True, extra_mode="Input", noise_avg=False)
SR_CFG = dict(im_chn=3, sigma_chn=1, kernel_chn=3, n_feat=[96, 160, 224], dep_S=5, dep_K=8, noise_cond=True, kernel_cond=True, n_resblocks=2,
              extra_mode="Both", noise_avg=True)


@pytest.fixture(autouse=True)
def _forms(monkeypatch):
    for k in ("VIRNET_WX4_MIN_TILES", "VIRNET_WX4_MIN_COUT", "VIRNET_WX4_MIN_FILL", "VIRNET_WINOGRAD", "VIRNET_RANGE_GUARD", "VIRNET_GUARD_CHECK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VIRNET_CONV_FORM", "wx4")
    monkeypatch.setenv("VIRNET_DETERMINISTIC", "1")
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")          # (net(x) eager: the comparisons are between two eager runs of the same kernels)


def _synth(cls, cfg, seed=0):
    net = cls(**cfg)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=seed), strict=True)
    return net.cuda().eval()


@pytest.fixture(scope="module")
def den():
    return _synth(VIRAttResUNet, DEN_CFG)


@pytest.fixture(scope="module")
def sr():
    return _synth(VIRAttResUNetSR, SR_CFG)


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.copy()).cuda()


# ---- the kernels against their definitions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_gather_is_gather_np_bit_for_bit_whatever_the_chunks(case):
    p, want, src = rc.plan_of(case), rc.gathered(case), _dev(rc.image(case))
    for chunk in (1, 5, p.T):
        got = torch.cat([restore.gather(src, p, a, min(a + chunk, p.T), layout=case[5]) for a in range(0, p.T, chunk)])
        assert rc.same_bits(got, want), chunk
    if case[4] == "u8" and case[5] == "hwc":             # a numpy image is uploaded as it is
        assert rc.same_bits(restore.gather(rc.image(case), p, 1, min(4, p.T)), want[1:4])


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("case", rc.BLEND_CASES, ids=rc.BLEND_IDS)
def test_blend_is_blend_np_bit_for_bit(case, scale):
    tiles = _dev(rc.stack(case, scale))
    for blend in restore.BLENDS:
        p = rc.plan_of(case, scale, blend)
        res = {}
        for out, layout in rc.OPTIONS:
            got = res[out, layout] = restore.blend(tiles, p, out=out, layout=layout)
            assert rc.same_bits(got, rc.blended(case, scale, blend, out, layout)), (blend, out, layout)
        for layout in restore.LAYOUTS:
            f = res["float32", layout].cpu().numpy()
            assert np.array_equal(res["uint8", layout].cpu().numpy(), veval.img_as_ubyte(np.clip(f, 0, 1))), (blend, layout)
        raw = restore.blend(tiles, p, out="float32", layout="chw", clip=False)
        assert rc.same_bits(raw, restore.blend_np(rc.stack(case, scale), p, out="float32", layout="chw", clip=False)), blend
        assert float(raw.min()) < 0 and float(raw.max()) > 1


def test_a_nan_tile_stays_inside_its_support_on_the_device():
    case = rc.CASES[0]
    tiles = rc.stack(case, 2).copy()
    tiles[9] = np.nan
    for blend in restore.BLENDS:
        p = rc.plan_of(case, 2, blend)
        got = restore.blend(_dev(tiles), p, out="float32", layout="chw")
        want = restore.blend_np(tiles, p, out="float32", layout="chw")
        assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want)) and rc.same_bits(torch.nan_to_num(got, nan=7.0), np.nan_to_num(want, nan=7.0))


def test_argument_errors_on_the_device():
    p = rc.plan_of(rc.CASES[0])
    with pytest.raises(ValueError, match="made for 37x53"):
        restore.gather(torch.zeros(38, 53, 3, dtype=torch.uint8, device="cuda"), p, 0, 1)
    with pytest.raises(TypeError, match="uint8 or float32"):
        restore.gather(torch.zeros(37, 53, 3, dtype=torch.float16, device="cuda"), p, 0, 1)
    with pytest.raises(ValueError, match=r"\[24,C,16,16\]"):
        restore.blend(torch.zeros(24, 3, 16, 17, device="cuda"), p)
    with pytest.raises(ValueError, match="forward must map"):
        restore.restore_tiles(lambda t: t[:, :, :8], torch.zeros(37, 53, 3, dtype=torch.uint8, device="cuda"), p)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_denoiser_crop_is_forward_tiled_and_linear_is_blend_np(den):
    x = synth_images(1, 3, 96, 80).cuda()
    with torch.no_grad():
        want_mu = forward_tiled(lambda t: den(t)[0], x, tile=32, overlap=8)
        want_sig = forward_tiled(lambda t: den(t)[1], x, tile=32, overlap=8)
        mu, sig = restore.restore_image(den, x[0], tile=32, overlap=8, blend="crop", out="float32", layout="chw", sigma=True, image_layout="chw",
                                        clip=False)
        assert mu.shape == (3, 96, 80) and sig.shape == (1, 96, 80)
        assert rc.same_bits(sig, want_sig[0].cpu().numpy()) and rc.same_bits(mu, want_mu[0].cpu().numpy())
        mu = restore.restore_image(den, x[0], tile=32, overlap=8, blend="crop", out="float32", layout="chw", image_layout="chw")
        assert torch.equal(mu, want_mu[0].clamp(0, 1))
        p = restore.plan(96, 80, 32, 8, multiple=4, blend="linear")
        stacks = restore.restore_tiles(lambda t: engine._denoise_forward(den, t), x[0], p, layout="chw")
        lin, lin_sig = restore.restore_image(den, x[0], tile=32, overlap=8, blend="linear", out="float32", layout="chw", sigma=True,
                                             image_layout="chw")
    assert rc.same_bits(lin, restore.blend_np(stacks[0].cpu().numpy(), p, out="float32", layout="chw"))
    assert rc.same_bits(lin_sig, restore.blend_np(stacks[1].cpu().numpy(), p, out="float32", layout="chw", clip=False))
    # outside the overlap bands (one covering tile along either axis) linear is crop; inside them it is not
    single = ((p.row_idx >= 0).sum(axis=1) == 1)[:, None] & ((p.col_idx >= 0).sum(axis=1) == 1)[None, :]
    a, b = lin.cpu().numpy(), mu.cpu().numpy()
    assert single.any() and not single.all()
    assert np.array_equal(a[:, single], b[:, single]) and (a[:, ~single] != b[:, ~single]).any()
    # uint8 in, uint8 out: the same tiles from the quantised image, quantised on the way out
    u8 = (x[0] * 255).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    with torch.no_grad():
        q = restore.restore_image(den, u8, tile=32, overlap=8)
        f = restore.restore_image(den, u8, tile=32, overlap=8, out="float32")
    assert q.dtype == torch.uint8 and q.shape == (96, 80, 3)
    assert np.array_equal(q.cpu().numpy(), veval.img_as_ubyte(f.cpu().numpy()))


def test_sisr_crop_is_forward_tiled_sisr(sr):
    x = synth_images(1, 3, 48, 40).cuda()
    with torch.no_grad():
        want_mu, want_k, want_s = forward_tiled_sisr(sr, x, 2, tile=32, overlap=8)
        mu, kinfo, sigma = restore.restore_image(sr, x[0], sf=2, tile=32, overlap=8, blend="crop", out="float32", layout="chw",
                                                 image_layout="chw", clip=False)
        lin = restore.restore_image(sr, x[0], sf=2, tile=32, overlap=8, out="float32", layout="chw", image_layout="chw")[0]
    assert mu.shape == (3, 96, 80)
    assert torch.equal(kinfo, want_k) and torch.equal(sigma, want_s)
    assert rc.same_bits(mu, want_mu[0].cpu().numpy())
    assert torch.isfinite(lin).all() and not torch.equal(lin, mu.clamp(0, 1))
    with pytest.raises(ValueError, match="too large for SNet / KNet"):
        restore.restore_image(sr, x[0], sf=2, image_layout="chw", limit_bytes=2 ** 18)


def test_auto_tile_with_a_small_limit_is_the_explicit_plan(den):
    x = synth_images(1, 3, 96, 80).cuda()
    tile = restore.auto_tile(96, 80, restore.widest_channels(den), 1, limit_bytes=2 ** 20, multiple=4)
    assert 0 < tile < 80
    with torch.no_grad():
        auto = restore.restore_image(den, x[0], tile="auto", overlap=8, image_layout="chw", limit_bytes=2 ** 20)
        explicit = restore.restore_image(den, x[0], tile=tile, overlap=8, image_layout="chw")
        assert torch.equal(auto, explicit) and auto.dtype == torch.uint8 and auto.shape == (96, 80, 3)
        # an image that fits: the plain forward, then the quantisation
        one = restore.restore_image(den, x[0], tile="auto", image_layout="chw", out="float32", layout="chw")
        assert torch.equal(one, den(x)[0][0].clamp(0, 1))
        assert torch.equal(restore.restore_image(den, x[0], tile="auto", image_layout="chw", layout="chw").cpu(),
                           torch.from_numpy(veval.img_as_ubyte(one.cpu().numpy())))


def test_testing_demo_restores_with_tile_auto(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    Image.fromarray(rng.integers(0, 256, (96, 80, 3), dtype=np.uint8)).save(tmp_path / "photo.png")
    out = tmp_path / "out"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "testing_demo.py"), "-i", str(tmp_path / "photo.png"), "-o", str(out),
                          "--tile", "auto", "--overlap", "8", "--blend", "linear", "--limit-bytes", str(2 ** 20)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "tile 52" in res.stdout, res.stdout
    with Image.open(out / "photo.png") as im:
        assert im.size == (80, 96) and im.mode == "RGB"


# ---- graph capture and the range guard ---------------------------------------------------------------------------------------------------
def test_gather_and_blend_replay_from_a_graph():
    case = rc.CASES[0]
    p = rc.plan_of(case)
    src = _dev(rc.image(case))
    p.tables(src.device)
    eager = restore.blend(restore.gather(src, p, 0, p.T), p, out="uint8", layout="hwc")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = restore.blend(restore.gather(src, p, 0, p.T), p, out="uint8", layout="hwc")
    for _ in range(2):
        got.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, eager)
    assert rc.same_bits(eager, restore.blend_np(rc.gathered(case), p, out="uint8", layout="hwc"))
    src.copy_(255 - src)                                  # the replay reads the source where it lies
    g.replay()
    assert torch.equal(got, restore.blend(restore.gather(src, p, 0, p.T), p, out="uint8", layout="hwc"))


def test_one_guard_decision_covers_the_image(sr):
    x = synth_images(1, 3, 40, 40).cuda()
    xh = x.clone()
    xh[0, :, 10:14, 10:14] = 3.0e4
    with torch.no_grad():
        with ops.forward_scope(form=engine.FP32_FORM):
            ref = restore.restore_image(sr, xh[0], sf=2, tile=32, overlap=8, out="float32", layout="chw", image_layout="chw")[0]
        engine.guard_stats(reset=True)
        with pytest.warns(RuntimeWarning, match="fp16's range"):
            mu, _, _ = restore.restore_image(sr, xh[0], sf=2, tile=32, overlap=8, out="float32", layout="chw", image_layout="chw")
        assert engine.guard_stats() == {"forwards": 1, "reruns": 1}
        assert bool(torch.isfinite(mu).all()) and torch.equal(mu, ref)
        engine.guard_stats(reset=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            restore.restore_image(sr, x[0], sf=2, tile=32, overlap=8, image_layout="chw")
        assert engine.guard_stats() == {"forwards": 1, "reruns": 0}
