"""CPU-side checks of the device metrics (virnet_amd/metrics.py, csrc/metrics.hip): the C ABI carries the new entries under the unchanged
version, the Python layer refuses bad arguments before it touches a device, and the evaluation tables' default path is the host path."""
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from virnet_amd import _native, eval as veval, metrics, sisr_eval

NEW_SYMBOLS = ("virnet_quantize_u8", "virnet_rgb2y_u8", "virnet_psnr_ssim_workspace_bytes", "virnet_psnr_ssim")


def test_new_symbols_bound_and_abi_version_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5


def test_window_taps_are_the_host_window():
    g = metrics.gauss_taps()
    assert g.dtype == np.float64 and g.shape == (11,)
    assert np.array_equal(np.outer(g, g), veval._gauss_window())


def test_workspace_size_and_geometry_errors_without_gpu():
    lib = _native.load()
    # 481 x 321: SSIM map 471 x 311 -> 15 x 10 tiles of 32 x 32, one fp64 + one 64-bit integer partial per tile and channel
    assert lib.virnet_psnr_ssim_workspace_bytes(2, 3, 481, 321, 0, 0) == 2 * 3 * 15 * 10 * 16
    assert lib.virnet_psnr_ssim_workspace_bytes(2, 3, 481, 321, 0, 1) == 2 * 1 * 15 * 10 * 16
    assert lib.virnet_psnr_ssim_workspace_bytes(1, 1, 43, 43, 16, 0) == 16
    for bad in [(1, 2, 32, 32, 0, 0), (1, 1, 32, 32, 0, 1), (1, 3, 32, 32, -1, 0), (0, 3, 32, 32, 0, 0), (1, 3, 8, 32, 4, 0)]:
        assert lib.virnet_psnr_ssim_workspace_bytes(*bad) == 0
        assert lib.virnet_last_error()


def test_psnr_from_sse_is_the_host_expression():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    b = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    sse = int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
    assert metrics.psnr_from_sse(sse, a.size) == veval.calculate_psnr(a, b)
    assert metrics.psnr_from_sse(0, a.size) == float("inf")


def test_psnr_ssim_refuses_bad_arguments_before_any_device_work():
    u8 = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    f32 = torch.zeros(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.psnr_ssim(u8, u8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.psnr_ssim(f32, u8)
    with pytest.raises(TypeError, match="uint8 or float32"):
        metrics.psnr_ssim(f32.double(), u8)
    with pytest.raises(TypeError, match="uint8 or float32"):
        metrics.psnr_ssim(u8, u8.to(torch.int32))
    with pytest.raises(ValueError, match="Input images must have the same dimensions."):
        metrics.psnr_ssim(u8, torch.zeros(1, 3, 32, 31, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\[N,C,H,W\]"):
        metrics.psnr_ssim(u8[0], u8[0])
    with pytest.raises(ValueError, match="smaller than the 11x11 SSIM window"):
        metrics.psnr_ssim(u8, u8, border=11)                  # 32 - 22 = 10 < 11
    with pytest.raises(ValueError, match="smaller than the 11x11 SSIM window"):
        metrics.psnr_ssim(torch.zeros(1, 3, 40, 10, dtype=torch.uint8), torch.zeros(1, 3, 40, 10, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # 10 x 10 is enough for PSNR alone
        metrics.psnr_ssim(u8, u8, border=11, with_ssim=False)
    with pytest.raises(ValueError, match="negative"):
        metrics.psnr_ssim(u8, u8, border=-1)
    with pytest.raises(ValueError, match="channels"):
        metrics.psnr_ssim(torch.zeros(1, 2, 32, 32, dtype=torch.uint8), torch.zeros(1, 2, 32, 32, dtype=torch.uint8))
    with pytest.raises(ValueError, match="ycbcr"):
        metrics.psnr_ssim(u8[:, :1], u8[:, :1], ycbcr=True)
    with pytest.raises(TypeError):
        metrics.to_uint8(u8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.to_uint8(f32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.rgb2y(u8)
    with pytest.raises(TypeError):
        metrics.rgb2y(f32)


def _two_images(tmp_path, folder, ext, crop=None):
    dst = tmp_path / folder
    dst.mkdir()
    files = sorted(f for f in os.listdir(os.path.join(GOLDEN, folder)) if f.endswith("." + ext))[:2]
    for f in files:
        if crop is None:
            shutil.copy(os.path.join(GOLDEN, folder, f), dst / f)
        else:
            from PIL import Image
            with Image.open(os.path.join(GOLDEN, folder, f)) as im:
                im.convert("RGB").crop((0, 0, crop[1], crop[0])).save(dst / f)
    return str(dst), [str(dst / f) for f in files]


def test_denoise_table_default_is_the_host_path(tmp_path):
    folder, files = _two_images(tmp_path, "cbsd68", "png", crop=(48, 64))

    def forward(noisy):
        return noisy * np.float32(0.9) + np.float32(0.03)

    rows = veval.denoise_table(forward, [folder + ":png"], noise_type="iid")
    again = veval.denoise_table(forward, [folder + ":png"], noise_type="iid", device_metrics=False)
    assert rows == again and [r["case"] for r in rows] == [15, 25, 50]
    rng = np.random.default_rng(seed=veval.NOISE_SEED)
    for row in rows:
        assert list(row) == ["dataset", "case", "psnr", "ssim", "images", "per_image_psnr"]
        psnrs, ssims = [], []
        for f in files:
            gt = veval.imread_rgb_uint8(f)
            noise = rng.standard_normal(size=gt.shape) * (np.ones(gt.shape[:2], dtype=np.float32) * (row["case"] / 255.0))[:, :, np.newaxis]
            den = veval.img_as_ubyte(np.clip(forward(veval.img_as_float32(gt) + noise.astype(np.float32)), 0.0, 1.0))
            psnrs.append(veval.calculate_psnr(den, gt))
            ssims.append(veval.calculate_ssim(den, gt))
        assert row["per_image_psnr"] == psnrs and row["psnr"] == float(np.mean(psnrs)) and row["ssim"] == float(np.mean(ssims))
        assert row["images"] == 2 and all(type(p) is float for p in row["per_image_psnr"])


def test_sisr_table_default_is_the_host_path(tmp_path):
    folder, files = _two_images(tmp_path, "set5", "bmp", crop=(96, 80))
    sf = 2
    kernels = sisr_eval.test_kernels(sf)[:2]

    def forward(lr, sf_):
        return np.repeat(np.repeat(lr, sf_, axis=0), sf_, axis=1)

    rows = sisr_eval.sisr_table(forward, [folder + ":bmp"], sf, kernels=kernels)
    assert rows == sisr_eval.sisr_table(forward, [folder + ":bmp"], sf, kernels=kernels, device_metrics=False)
    for row, kernel in zip(rows, kernels):
        assert list(row) == ["dataset", "kernel", "psnr_y", "ssim_y", "images", "per_image_psnr_y"]
        psnrs, ssims = [], []
        for f in files:
            gt = sisr_eval.modcrop(veval.imread_rgb_uint8(f), sf)
            sr = veval.img_as_ubyte(np.clip(forward(sisr_eval.degrade(veval.img_as_float32(gt), kernel, sf), sf), 0.0, 1.0))
            psnrs.append(veval.calculate_psnr_y(sr, gt, border=sf ** 2))
            ssims.append(veval.calculate_ssim(sr, gt, border=sf ** 2, ycbcr=True))
        assert row["per_image_psnr_y"] == psnrs and row["psnr_y"] == float(np.mean(psnrs)) and row["ssim_y"] == float(np.mean(ssims))


def test_device_metrics_refuses_a_host_forward(tmp_path):
    folder, _ = _two_images(tmp_path, "cbsd68", "png", crop=(32, 32))
    with pytest.raises(TypeError, match="CUDA tensor"):
        veval.denoise_table(lambda noisy: noisy, [folder + ":png"], noise_type="iid", device_metrics=True)
    with pytest.raises(RuntimeError, match="CUDA"):
        veval.denoise_table(lambda noisy: torch.from_numpy(noisy.transpose(2, 0, 1).copy()), [folder + ":png"], noise_type="iid",
                            device_metrics=True)
