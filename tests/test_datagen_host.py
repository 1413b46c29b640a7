"""CPU-side checks of the batch synthesis (virnet_amd/datagen.py): the generator's known answers and moments, the parameter drawers and the
numpy definitions against batches that the reference's own dataset classes produced (tests/golden/datagen.npz, written by
tests/golden/make_datagen_golden.py), the two uint8 conversions on all 256 values, the bindings and the argument errors.  No kernel runs."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, load_golden
from datagen_cases import ulps
from virnet_amd import _native, datagen
from virnet_amd import eval as veval

NEW_SYMBOLS = ("virnet_datagen_patches", "virnet_datagen_normal", "virnet_datagen_blur_kernels")
P, HR, K = 32, 48, 21


@pytest.fixture(scope="module")
def G():
    g = load_golden("datagen")
    g["seed_of"] = dict(zip(g["seed_names"].tolist(), g["seeds"].tolist()))
    return g


def _images(names):
    return [veval.imread_rgb_uint8(os.path.join(GOLDEN, "cbsd68", str(n))) for n in names]


# ---- the generator ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_philox_known_answers(counter, key, want):
    got = datagen.philox4x32_np(np.asarray(counter, dtype=np.uint32), np.asarray(key, dtype=np.uint32))
    assert got.dtype == np.uint32 and got.tolist() == want


def test_normal_np_moments():
    n = 1 << 22
    z = datagen.normal_np((1, n), 1234, [7]).reshape(-1)
    assert z.dtype == np.float64 and np.isfinite(z).all()
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    stats = abs(mean) * np.sqrt(n), abs(var - 1) * np.sqrt(n / 2), abs(kurt - 3) * np.sqrt(n / 24)
    print("normal_np: |mean| sqrt(n) %.3f, |var - 1| sqrt(n/2) %.3f, |kurtosis - 3| sqrt(n/24) %.3f" % stats)
    assert all(s < 4 for s in stats)


def test_normal_np_depends_on_the_sample_id_alone_and_takes_normal_e_and_3():
    a = datagen.normal_np((3, 2, 5), 9, [4, 5, 6], stream=1)
    b = datagen.normal_np((2, 2, 5), 9, [6, 4], stream=1)
    assert np.array_equal(a[2], b[0]) and np.array_equal(a[0], b[1])
    assert not np.array_equal(a, datagen.normal_np((3, 2, 5), 9, [4, 5, 6], stream=0))
    assert not np.array_equal(a, datagen.normal_np((3, 2, 5), 10, [4, 5, 6], stream=1))
    # element e of a sample: normal e & 3 of counter e >> 2, by the stated formula
    w = datagen.normal_words_np(10, 9, [4], 1)[0]
    for e in (0, 1, 2, 3, 6, 9):
        w1, w2 = w[e >> 2, (e & 2)], w[e >> 2, (e & 2) + 1]
        u1, u2 = ((int(w1) >> 8) + 1) * 2.0 ** -24, (int(w2) >> 8) * 2.0 ** -24
        r = np.sqrt(-2 * np.log(u1))
        want = r * (np.sin(2 * np.pi * u2) if e & 1 else np.cos(2 * np.pi * u2))
        assert a[0].reshape(-1)[e] == want
    f32 = datagen.normal_np((3, 2, 5), 9, [4, 5, 6], stream=1, dtype=np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - a).max() < 1e-5


# ---- the uint8 conversions ------------------------------------------------------------------------------------------------------------------
def test_both_uint8_conversions_on_all_256_values():
    v = np.arange(256, dtype=np.uint8)
    mul, div = datagen.u8_to_float_np(v), datagen.u8_to_float_np(v, divide=True)
    assert mul.dtype == div.dtype == np.float32
    assert np.array_equal(mul, veval.img_as_float32(v)) and np.array_equal(mul, v.astype(np.float32) * np.float32(1.0 / 255.0))
    # the division is the correctly rounded quotient (255 q is exact in fp64 for an fp32 q, so the two neighbours can be compared exactly)
    q = div.astype(np.float64)
    for cand in (np.nextafter(div, np.float32(2)), np.nextafter(div, np.float32(-1))):
        assert (np.abs(q * 255.0 - v) <= np.abs(cand.astype(np.float64) * 255.0 - v)).all()
    assert mul[0] == div[0] == 0.0 and mul[255] == div[255] == 1.0
    assert int((mul != div).sum()) == 126 and np.abs(mul.astype(np.float64) - q).max() <= 2.0 ** -24
    assert (np.diff(mul) > 0).all() and (np.diff(div) > 0).all()


# ---- the reference's own batches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode,clip", [("niid", "niid", False), ("iid", "iid", False), ("clip", "niid", True)])
def test_denoise_definition_against_the_reference_dataset(G, case, mode, clip):
    images = _images(G["den_files"])
    want_noisy, want_gt, want_sigma = (G[f"den_{case}_{k}"] for k in ("noisy", "gt", "sigma"))
    n = want_gt.shape[0]
    params = datagen.draw_denoise_params(random.Random(G["seed_of"][f"den_{case}"]), images, n, P, mode)
    noise = np.ascontiguousarray(G[f"den_{case}_randn"].transpose(0, 3, 1, 2))
    noisy, gt, sigma = datagen.denoise_batch_np(images, params, noise, clip)
    assert noisy.dtype == gt.dtype == sigma.dtype == np.float32 and sigma.shape == (n, 1, P, P)
    assert np.array_equal(gt.view(np.uint32), want_gt.view(np.uint32))          # also pins the drawers: index, offsets, flag
    # one ulp on the map, doubled by the square, plus its rounding
    u = ulps(sigma, want_sigma)
    # |noise| <= 6 times one ulp of a sigma <= 80/255, plus two roundings at magnitude <= 4
    err = np.abs(noisy.astype(np.float64) - want_noisy)
    print(f"{case}: sigma_map_gt max {u.max():.2f} ulp, {float((u > 0).mean()):.2%} differ; im_noisy max err {err.max():.2e}, "
          f"{float((err > 0).mean()):.2%} differ")
    assert u.max() <= 4 and err.max() <= 5e-7
    if clip:
        assert noisy.min() >= 0.0 and noisy.max() <= 1.0 and (noisy == 0.0).any()
    assert len(set(params.flag.tolist())) > 1 or n < 3


def test_sigma_map_without_a_reduction_is_the_reference_formula():
    rng = random.Random(5)
    differ = total = 0
    for p in (16, 33):
        for _ in range(20):
            c = [rng.uniform(0, p), rng.uniform(0, p)]
            scale, up, down = rng.uniform(p / 4, p / 4 * 3), rng.uniform(0.1, 0.3), rng.uniform(0.0, 0.1)
            ii, jj = [x.astype(np.float64) for x in np.meshgrid(np.arange(p), np.arange(p), indexing="ij")]
            kk = np.exp((-(ii - c[0]) ** 2 - (jj - c[1]) ** 2) / (2 * scale ** 2))       # DenoisingDatasets.py:190-203 with util_denoising.py:12-22
            kk /= kk.sum()
            want = (down + (kk - kk.min()) / (kk.max() - kk.min()) * (up - down)).astype(np.float32)
            got = datagen.sigma_map_np(p, c[0], c[1], scale, up, down)
            differ += int((got != want).sum())
            total += want.size
            assert ulps(got, want).max() <= 1
    print(f"sigma map: {differ} of {total} fp32 elements differ from the formula with the reduction")


@pytest.mark.parametrize("case,sf,down", [("sf2", 2, "direct"), ("sf4", 4, "bicubic")])
def test_sisr_definition_against_the_reference_dataset(G, case, sf, down):
    images = _images(G["sisr_files"])
    params = datagen.draw_sisr_params(random.Random(G["seed_of"][f"sisr_{case}"]), images, 4, HR, sf)
    noise = np.ascontiguousarray(G[f"sisr_{case}_randn"].transpose(0, 3, 1, 2))
    im_hr, im_lr, im_blur, kinfo, nlevel = datagen.sisr_batch_np(images, params, sf, K, noise, down)
    assert np.array_equal(im_hr.view(np.uint32), G[f"sisr_{case}_hr"].view(np.uint32))
    assert np.array_equal(nlevel.view(np.uint32), G[f"sisr_{case}_nlevel"].view(np.uint32)) and nlevel.shape == (4, 1, 1, 1)
    assert ulps(kinfo, G[f"sisr_{case}_kinfo"]).max() <= 1
    # the bar tests/test_jpeg_host.py holds the degradation's host definition to against the reference's output
    e_blur, e_lr = np.abs(im_blur - G[f"sisr_{case}_blur"]).max(), np.abs(im_lr - G[f"sisr_{case}_lr"]).max()
    print(f"{case}: im_blur max err {e_blur:.2e}, im_lr max err {e_lr:.2e}")
    assert e_blur <= 1e-6 and e_lr <= 1e-6
    assert (params.lam2 == params.lam1).any() or (params.lam2 != params.lam1).all()


def test_blur_kernels_np_is_the_pinned_host_definition():
    H = load_golden("sisr_harness")
    spec = [(0.40, 0.40, 0.0), (0.60, 0.60, 0.0), (0.80, 0.80, 0.0), (0.4, 0.2, 0.0), (0.6, 0.3, 0.75 * np.pi), (0.8, 0.4, 0.25 * np.pi),
            (0.8, 0.4, 0.50 * np.pi)]
    for sf in (2, 3, 4):
        kernel, kinfo = datagen.blur_kernels_np([(a * sf) ** 2 for a, _, _ in spec], [(b * sf) ** 2 for _, b, _ in spec], [t for _, _, t in spec], 21, sf)
        assert kernel.shape == (7, 1, 21, 21) and kernel.dtype == np.float32 and kinfo.shape == (7, 3)
        assert ulps(kernel[:, 0], H[f"kernels_sf{sf}"].astype(np.float32)).max() <= 1
    kernel, kinfo = datagen.blur_kernels_np([1.2], [5.0], [0.3], 21, 4, shift=True)
    assert ulps(kernel[0, 0], H["shifted_kernel"].astype(np.float32)).max() <= 1 and ulps(kinfo[0], H["shifted_info"].astype(np.float32)).max() <= 1


def test_sisr_drawer_consumes_the_stream_like_the_reference_with_jpeg():
    """add_jpeg: random.sample picks the type, a JPEG sample draws its quality (two randints) before its std"""
    shapes = [(60, 70), (50, 50)]
    rng, twin = random.Random(21), random.Random(21)
    params = datagen.draw_sisr_params(rng, shapes, 12, HR, 3, add_jpeg=True)
    for i in range(12):
        ind = twin.randint(0, 1)
        h, w = shapes[ind]
        got = (ind, twin.randint(0, h - HR), twin.randint(0, w - HR), twin.randint(0, 7))
        assert got == (params.img[i], params.ind_h[i], params.ind_w[i], params.flag[i])
        lam1 = twin.uniform(0.2, 3)
        lam2 = twin.uniform(lam1, 3) if twin.random() < 0.7 else lam1
        theta = twin.uniform(0, np.pi)
        kind = twin.sample(["Gaussian", "JPEG"], k=1)[0]
        if kind == "JPEG":
            start, end = list(range(30, 50, 5)) + [60, 70, 80], list(range(35, 50, 5)) + [60, 70, 80, 95]
            r = twin.randint(0, len(start) - 1)
            qf, std = twin.randint(start[r], end[r]), twin.uniform(0.1, 10) / 255.0
        else:
            qf, std = 0, twin.uniform(0.1, 15) / 255.0
        assert (lam1, lam2, theta, std, qf) == (params.lam1[i], params.lam2[i], params.theta[i], params.std[i], params.qf[i])
    assert rng.random() == twin.random() and 0 < int((params.qf > 0).sum()) < 12


def test_pair_drawer_and_definition():
    g = np.random.default_rng(3)
    noisy = [g.integers(0, 256, (40, 37, 3), dtype=np.uint8), g.integers(0, 256, (33, 52, 3), dtype=np.uint8)]
    gt = [g.integers(0, 256, im.shape, dtype=np.uint8) for im in noisy]
    rng, twin = random.Random(2), random.Random(2)
    params = datagen.draw_pair_params(rng, noisy, 10, 33)
    a, b = datagen.pair_batch_np(noisy, gt, params)
    for i in range(10):
        ind = twin.randint(0, 1)
        y, x = twin.randint(0, noisy[ind].shape[0] - 33), twin.randint(0, noisy[ind].shape[1] - 33)
        flag = twin.randint(0, 7)
        for got, ims in ((a, noisy), (b, gt)):
            want = veval.img_as_float32(ims[ind][y:y + 33, x:x + 33])
            want = np.rot90(want, k=flag >> 1)
            want = np.flipud(want) if flag & 1 else want
            assert np.array_equal(got[i], want.transpose(2, 0, 1))
    assert rng.random() == twin.random()


def test_pack_layout():
    params = datagen.draw_sisr_params(random.Random(1), [(50, 60)], 3, HR, 2, add_jpeg=True)
    blob = params.pack()
    n = 3
    assert blob.dtype == np.uint8 and blob.shape == (datagen.RECORD_BYTES * n,)
    i32, f64 = blob[:32 * n].view(np.int32).reshape(8, n), blob[32 * n:].view(np.float64).reshape(8, n)
    assert np.array_equal(i32[:4], np.stack([params.img, params.ind_h, params.ind_w, params.flag])) and np.array_equal(i32[5], params.qf)
    assert np.array_equal(blob[24 * n:28 * n].view(np.float32), params.std.astype(np.float32))
    assert np.array_equal(f64[5], params.lam1 ** 2) and np.array_equal(f64[6], params.lam2 ** 2) and np.array_equal(f64[7], params.theta)
    den = datagen.draw_denoise_params(random.Random(1), [(50, 60)], n, P)
    f64 = den.pack()[32 * n:].view(np.float64).reshape(8, n)
    assert np.array_equal(f64[2], [2 * s ** 2 for s in den.scale.tolist()]) and np.array_equal(f64[3], den.down) and np.array_equal(f64[4], den.up)


# ---- bindings and argument errors ---------------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_the_abi_version_is_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5
    header = open(os.path.join(REPO, "include", "virnet_hip.h")).read()
    assert f"#define VIRNET_DATAGEN_MAX_PATCH {datagen.MAX_PATCH}\n" in header and f"#define VIRNET_DATAGEN_MAX_KERNEL {datagen.MAX_KERNEL}\n" in header
    for name, value in (("DENOISE", datagen.DENOISE), ("PAIR", datagen.PAIR), ("HR", datagen.HR)):
        assert f"#define VIRNET_DATAGEN_{name} {value}\n" in header


def test_argument_errors():
    g = np.random.default_rng(0)
    images = [g.integers(0, 256, (40, 50, 3), dtype=np.uint8), g.integers(0, 256, (36, 36, 3), dtype=np.uint8)]
    rng = random.Random(0)
    with pytest.raises(ValueError, match="smaller than the 37x37 patch.*cv2.resize.*out of scope"):      # patch larger than an image
        datagen.draw_denoise_params(rng, images, 2, 37)
    with pytest.raises(ValueError, match="smaller than"):
        datagen.draw_sisr_params(rng, images, 2, 41, 2)
    ok = dict(img=[0, 1], ind_h=[4, 0], ind_w=[14, 0], flag=[7, 0])
    datagen.BatchParams(images, 36, **ok)
    with pytest.raises(ValueError, match="flag 8"):
        datagen.BatchParams(images, 36, **dict(ok, flag=[8, 0]))
    with pytest.raises(ValueError, match="past the edge"):
        datagen.BatchParams(images, 36, **dict(ok, ind_w=[15, 0]))
    with pytest.raises(ValueError, match="past the edge"):
        datagen.BatchParams(images, 36, **dict(ok, ind_h=[4, 1]))
    with pytest.raises(ValueError, match="past the edge"):
        datagen.BatchParams(images, 36, **dict(ok, ind_h=[-1, 0]))
    with pytest.raises(ValueError, match="image index 2"):
        datagen.BatchParams(images, 36, **dict(ok, img=[0, 2]))
    with pytest.raises(TypeError, match="uint8"):
        datagen.ImagePool([images[0].astype(np.float32)], "cpu")
    with pytest.raises(ValueError, match="shapes"):
        datagen.ImagePool.paired(images, images[::-1], "cpu")
    with pytest.raises(ValueError, match="flag"):
        datagen.augment_np(images[0], 8)
    # CPU tensors: the package's usual error, raised before any device work; shape errors come first
    pool = datagen.ImagePool(images, "cpu")
    params = datagen.draw_denoise_params(rng, pool, 2, 36)
    with pytest.raises(ValueError, match=r"noise must be \(2, 3, 36, 36\)"):
        datagen.denoise_batch(pool, params, 36, 1, noise=torch.zeros(2, 3, 36, 35))
    with pytest.raises(TypeError, match="float32"):
        datagen.denoise_batch(pool, params, 36, 1, noise=torch.zeros(2, 3, 36, 36, dtype=torch.float64))
    with pytest.raises(ValueError, match="patch size 32"):
        datagen.denoise_batch(pool, params, 32, 1)
    with pytest.raises(ValueError, match="another pool"):
        datagen.denoise_batch(datagen.ImagePool(images[:1], "cpu"), params, 36, 1)
    for call in (lambda: datagen.denoise_batch(pool, params, 36, 1), lambda: datagen.denoise_batch(pool, params, 36, 1, noise=torch.zeros(2, 3, 36, 36)),
                 lambda: datagen.hr_batch(pool, params, 36), lambda: datagen.sisr_batch(pool, params, 36, 2),
                 lambda: datagen.pair_batch(datagen.ImagePool.paired(images, images, "cpu"), params, 36),
                 lambda: datagen.normal((2, 3), 1, device="cpu"), lambda: datagen.normal((2, 3), 1, sample_ids=torch.zeros(2, dtype=torch.int64)),
                 lambda: datagen.blur_kernels(*(torch.ones(2, dtype=torch.float64),) * 3), lambda: params.to("cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="second buffer"):
        datagen.pair_batch(pool, params, 36)
    with pytest.raises(ValueError, match="LR shape"):
        datagen.sisr_batch(pool, params, 36, 2, noise=torch.zeros(2, 3, 18, 17))
    with pytest.raises(TypeError, match="seed"):
        datagen.denoise_batch(pool, params, 36, seed=1.5)
    with pytest.raises(ValueError, match="odd sizes"):
        datagen.blur_kernels(*(torch.ones(2, dtype=torch.float64),) * 3, k_size=27)
