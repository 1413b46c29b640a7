"""Host side of the self-ensemble (virnet_amd/ensemble.py, virnet_amd/real_eval.py): the numpy definitions equal the scripts' literal
expressions, the shared cases hold what they promise, the new symbols are bound and bad arguments are refused.  No device needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ensemble_cases as ec
from conftest import REPO
from virnet_amd import _native, ensemble, real_eval
from virnet_amd import eval as veval

NEW_SYMBOLS = ("virnet_ensemble_expand", "virnet_ensemble_reduce")


def test_symbols_are_bound_and_the_abi_version_is_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
    assert lib.virnet_abi_version() == _native.ABI_VERSION == 5
    header = open(os.path.join(REPO, "include", "virnet_hip.h")).read()
    assert re.search(r"#define\s+VIRNET_ABI_VERSION\s+5\b", header)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header)


def test_library_rejects_bad_arguments_without_launching():
    lib = _native.load()
    p = ctypes.c_void_p(256)                    # never dereferenced: every call below is refused before the launch
    bad = [dict(c=2), dict(c=0), dict(b=0), dict(h=0), dict(w=-1), dict(modes=4), dict(b=70000)]
    for kw in bad:
        a = dict(b=1, h=4, w=4, c=3, modes=8)
        a.update(kw)
        assert lib.virnet_ensemble_expand(p, 0, p, p, a["b"], a["h"], a["w"], a["c"], a["modes"], None) != 0, kw
        assert b"virnet_ensemble_expand" in lib.virnet_last_error()
        assert lib.virnet_ensemble_reduce(p, p, p, 0, 0, 0, a["b"], a["h"], a["w"], a["c"], a["modes"], None) != 0, kw
        assert b"virnet_ensemble_reduce" in lib.virnet_last_error()
    assert lib.virnet_ensemble_expand(None, 0, p, p, 1, 4, 4, 3, 8, None) != 0 and b"NULL" in lib.virnet_last_error()
    assert lib.virnet_ensemble_expand(p, 0, p, None, 1, 4, 4, 3, 8, None) != 0 and b"NULL" in lib.virnet_last_error()
    assert lib.virnet_ensemble_reduce(p, None, p, 0, 0, 0, 1, 4, 4, 3, 8, None) != 0 and b"NULL" in lib.virnet_last_error()
    assert lib.virnet_ensemble_reduce(p, p, None, 0, 0, 0, 1, 4, 4, 3, 1, None) != 0 and b"NULL" in lib.virnet_last_error()


def test_python_argument_validation():
    u8 = np.zeros((1, 4, 4, 3), dtype=np.uint8)
    for f in (ensemble.expand, ensemble.expand_np):
        with pytest.raises(ValueError, match="channels"):
            f(np.zeros((1, 4, 4, 2), dtype=np.uint8))
        with pytest.raises(TypeError, match="uint8 or float32"):
            f(u8.astype(np.float64))
        with pytest.raises(ValueError, match=r"\[B,H,W,C\]"):
            f(u8[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ensemble.expand(torch.from_numpy(u8))
    with pytest.raises(TypeError, match="uint8 or float32"):
        ensemble.expand(torch.zeros(1, 4, 4, 3, dtype=torch.float16))
    even, odd = torch.zeros(4, 3, 5, 6), torch.zeros(4, 3, 6, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ensemble.reduce(even, odd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ensemble.reduce(even, None)
    with pytest.raises(ValueError, match="odd is"):
        ensemble.reduce(even, torch.zeros(4, 3, 5, 6))
    with pytest.raises(ValueError, match="odd is"):
        ensemble.reduce_np(even.numpy(), np.zeros((8, 3, 6, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="four orientations"):
        ensemble.reduce(torch.zeros(3, 3, 5, 6), torch.zeros(3, 3, 6, 5))
    with pytest.raises(TypeError, match="float32"):
        ensemble.reduce(even.double(), odd.double())
    with pytest.raises(ValueError, match="channels"):
        ensemble.reduce(torch.zeros(4, 2, 5, 6), torch.zeros(4, 2, 6, 5))
    for kw in (dict(order="tree"), dict(out="int8"), dict(layout="nhwc")):
        with pytest.raises(ValueError, match="expected one of"):
            ensemble.reduce(even, odd, **kw)
    with pytest.raises(ValueError, match="batch"):
        ensemble.restore_np(lambda x: x, u8, batch=0)
    with pytest.raises(ValueError, match="uint8"):
        real_eval.sidd_blocks_np(lambda x: x, u8)
    with pytest.raises(ValueError, match="float32"):
        real_eval.dnd_box_np(lambda x: x, u8[0])


def test_uint8_sources_become_the_correctly_rounded_quotient():
    """np.float32(u / 255.0) -- img_as_float's float64 division, then float32 -- and not eval.img_as_float32's float32 multiply."""
    u = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    even, _ = ensemble.expand_np(u)
    want = np.float32(u[0, :, :, 0] / 255.0)
    assert even.dtype == np.float32 and (ec.bits(even[0, 0]) == ec.bits(want)).all()
    assert (np.float32(np.arange(256) / 255.0) == np.arange(256, dtype=np.float32) / np.float32(255.0)).all()     # one IEEE fp32 division
    differs = veval.img_as_float32(u[0, :, :, 0]) != want
    assert int(differs.sum()) == 126
    assert (ensemble.expand_np(u, flip=False)[0][0, 0] == want).all()
    f = ec.source_f32((5, 3, 3, 1))
    assert (ec.bits(ensemble.expand_np(f, flip=False)[0][0].transpose(1, 2, 0)) == ec.bits(f[0])).all()      # float32 passes bit for bit


def test_case_file_holds_what_it_promises():
    seen = set()
    for case in ec.CASES:
        u = ec.source_u8(case)
        seen |= set(np.unique(u).tolist())
        if u.size >= 256:
            assert len(np.unique(u)) == 256
    assert len(seen) == 256
    case = (36, 52, 3, 3)
    o = ec.octets(case).reshape(-1, 8)
    seq, pair = ec.sums(case)
    assert int((seq != pair).sum()) >= 100                                   # octets whose two orders differ
    assert (o < 0).any() and (o > 1).any() and (o.max(axis=1) < 0).any() and (o.min(axis=1) > 1).any()
    zero = (o == 0).all(axis=1)
    neg = np.signbit(o).all(axis=1)
    assert (zero & neg).any() and (zero & ~np.signbit(o).any(axis=1)).any() and (zero & ~neg & np.signbit(o).any(axis=1)).any()
    mean = (seq / np.float32(8)).astype(np.float64)
    frac = mean * 255.0 - np.floor(mean * 255.0)                              # position between two byte values, 0.5 = a tie
    near = (np.abs(frac - 0.5) < 255.0 * 2.0 ** -23) & (mean > 0) & (mean < 1)          # within about an ulp of a tie
    assert (near & (frac < 0.5)).any() and (near & (frac > 0.5)).any()
    grid = np.isin(o, np.float32(np.arange(256) / 255.0)).all(axis=1) & ~(o == o[:, :1]).all(axis=1)
    assert (near & grid).any()                                                # ... some of them built from distinct byte-grid values


@pytest.mark.parametrize("case", [(5, 3, 3, 1), (33, 31, 1, 3), (36, 52, 3, 3)], ids=lambda c: "x".join(map(str, c)))
def test_definitions_equal_the_literal_script_expressions(case):
    h, w, c, b = case
    src = ec.source_u8(case)
    even, odd = ec.expanded(case, "u8")
    assert even.shape == (4 * b, c, h, w) and odd.shape == (4 * b, c, w, h) and even.dtype == odd.dtype == np.float32
    r_even, r_odd = ec.restored(case)
    for i in range(b):
        # scripts/denoising_virnet_real_sidd.py:121-136 with the forward replaced by "look the restored orientation up"
        acc = np.zeros((h, w, c), dtype=np.float32)
        stack = np.zeros((h, w, c, 8), dtype=np.float32)
        for flag in range(8):
            im = (veval.dihedral(src[i], flag) / 255.0).transpose((2, 0, 1))[np.newaxis]                  # img_as_float(data_aug_np(.))
            im = torch.from_numpy(im).type(torch.float32).numpy()
            group, j = (even, ensemble.EVEN_MODES.index(flag)) if flag in ensemble.EVEN_MODES else (odd, ensemble.ODD_MODES.index(flag))
            assert (ec.bits(group[i * 4 + j]) == ec.bits(im[0])).all()
            rgroup = r_even if flag in ensemble.EVEN_MODES else r_odd
            back = veval.dihedral_inverse(rgroup[i * 4 + j].transpose((1, 2, 0)), flag)
            assert (ec.bits(back) == ec.bits(ec.octets(case)[i, :, :, :, flag])).all()
            acc += back
            stack[:, :, :, flag] = back
        acc /= 8
        mean = stack.mean(axis=3, keepdims=False)
        assert (ec.bits(ec.reduced(case, "sequential", "uint8", "hwc")[i]) == veval.img_as_ubyte(acc.clip(0, 1))).all()
        assert (ec.bits(ec.reduced(case, "pairwise", "float32", "hwc")[i]) == ec.bits(np.clip(mean, 0.0, 1.0))).all()
        assert (ec.bits(ec.reduced(case, "sequential", "float32", "chw")[i]) == ec.bits(acc.clip(0, 1).transpose(2, 0, 1))).all()
        assert (ec.bits(ec.reduced(case, "pairwise", "uint8", "chw")[i]) == veval.img_as_ubyte(np.clip(mean, 0.0, 1.0)).transpose(2, 0, 1)).all()
        plain = r_even[i].transpose(1, 2, 0)
        assert (ec.bits(ec.reduced(case, "sequential", "float32", "hwc", False)[i]) == ec.bits(np.clip(plain, 0.0, 1.0))).all()
        assert (ec.reduced(case, "pairwise", "uint8", "hwc", False)[i] == veval.img_as_ubyte(plain.clip(0, 1))).all()
    # the arithmetic the kernel spells out: +0 start, then the two orders, one exact scaling
    seq, pair = ec.sums(case)
    assert (ec.bits(ec.reduced(case, "sequential", "float32", "hwc").reshape(-1)) == ec.bits(np.clip(seq / np.float32(8), 0.0, 1.0))).all()
    assert (ec.bits(ec.reduced(case, "pairwise", "float32", "hwc").reshape(-1)) == ec.bits(np.clip(pair / np.float32(8), 0.0, 1.0))).all()
    assert (seq / np.float32(8) != pair / np.float32(8)).any()


def test_restore_np_with_the_identity_forward_returns_the_source_bytes():
    for case in [(1, 1, 1, 1), (5, 3, 3, 3), (33, 31, 3, 1), (36, 52, 1, 3)]:
        src = ec.source_u8(case)
        for order in ensemble.ORDERS:
            for batch in (1, 3, 8):
                assert (ensemble.restore_np(lambda x: x, src, order=order, batch=batch) == src).all()
        assert (ensemble.restore_np(lambda x: x, src, flip=False) == src).all()
        assert (ensemble.restore_np(lambda x: x, src, layout="chw") == src.transpose(0, 3, 1, 2)).all()
        f = np.clip(ec.source_f32(case), 0, 1)
        got = ensemble.restore_np(lambda x: x, f, out="float32", order="pairwise")
        assert (got == f).all()                                               # (eight equal values: the mean is exact)


def test_restore_np_is_the_host_flip_ensemble():
    """eval.flip_ensemble (the helper the device path replaces) around the same forward gives the float result before the clip."""
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, size=(1, 9, 7, 3), dtype=np.uint8)
    k = rng.random((3, 1, 1), dtype=np.float32)
    fwd = lambda x: x * k + np.roll(x, 1, axis=3) * np.float32(0.25)          # noqa: E731  (not symmetric: the orientations differ)
    hwc = lambda a: fwd(np.ascontiguousarray(a.transpose(2, 0, 1))[None])[0].transpose(1, 2, 0)     # noqa: E731
    want = veval.flip_ensemble(hwc, np.float32(src[0] / 255.0))
    got = ensemble.restore_np(fwd, src, out="float32")
    assert (ec.bits(got[0]) == ec.bits(np.clip(want, 0.0, 1.0))).all()
    assert (ensemble.restore_np(fwd, src)[0] == veval.img_as_ubyte(np.clip(want, 0, 1))).all()


def test_sidd_blocks_np_on_a_mat_pair(tmp_path):
    import scipy.io as sio
    rng = np.random.default_rng(5)
    gt = rng.integers(0, 256, size=(2, 2, 16, 16, 3), dtype=np.uint8)
    noisy = np.clip(gt.astype(np.int32) + rng.integers(-20, 21, size=gt.shape), 0, 255).astype(np.uint8)
    sio.savemat(str(tmp_path / "ValidationNoisyBlocksSrgb.mat"), {"ValidationNoisyBlocksSrgb": noisy})
    sio.savemat(str(tmp_path / "ValidationGtBlocksSrgb.mat"), {"ValidationGtBlocksSrgb": gt})
    noisy_l = sio.loadmat(str(tmp_path / "ValidationNoisyBlocksSrgb.mat"))["ValidationNoisyBlocksSrgb"]
    gt_l = sio.loadmat(str(tmp_path / "ValidationGtBlocksSrgb.mat"))["ValidationGtBlocksSrgb"]
    assert noisy_l.dtype == np.uint8 and (noisy_l == noisy).all() and (gt_l == gt).all()
    fwd = lambda x: x * np.float32(0.9) + np.roll(x, 1, axis=2) * np.float32(0.1)                  # noqa: E731
    for flip in (True, False):
        res = real_eval.sidd_blocks_np(fwd, noisy_l, gt_l, flip=flip)
        den = res["denoised"]
        assert den.shape == noisy.shape and den.dtype == np.uint8 and res["psnr"].shape == res["ssim"].shape == (2, 2)
        psnr_all = ssim_all = 0
        for i in range(2):
            for k in range(2):
                assert res["psnr"][i, k] == veval.calculate_psnr(gt[i, k], den[i, k], border=0)
                assert res["ssim"][i, k] == veval.calculate_ssim(gt[i, k], den[i, k], border=0)
                psnr_all += res["psnr"][i, k]
                ssim_all += res["ssim"][i, k]
                assert (den[i, k] == ensemble.restore_np(fwd, noisy[i, k][None], flip)[0]).all()
        assert res["psnr_mean"] == psnr_all / 4 and res["ssim_mean"] == ssim_all / 4
    assert set(real_eval.sidd_blocks_np(fwd, noisy_l)) == {"denoised"}
    crop = rng.random((9, 7, 3), dtype=np.float32)
    assert (ec.bits(real_eval.dnd_box_np(fwd, crop)) == ec.bits(ensemble.restore_np(fwd, crop[None], True, "pairwise", "float32", "hwc")[0])).all()
