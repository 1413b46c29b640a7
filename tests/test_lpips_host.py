"""Host side of LPIPS (virnet_amd/lpips.py): the new symbols are bound, the weight loader reads both key layouts and refuses by name, the
torch definition equals an independent numpy restatement in fp64, and sisr_table's ``lpips=`` option adds its two keys last.  No device."""
import copy
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

import lpips_cases as lc
from conftest import REPO
from virnet_amd import _native, lpips, sisr_eval
from virnet_amd import eval as veval

NEW_SYMBOLS = ("virnet_lpips_workspace_bytes", "virnet_lpips", "virnet_lpips_features")
# both sides fp64, same operations, different summation order: K <= 3456 products of magnitude <= ~1 -> ~1e-13 relative at worst
FP64_REL = 1e-12


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
    assert header.count("scripts/sisr_virnet_syn.py:158-161") >= 3          # every entry cites the reference
    assert ctypes.sizeof(_native.LpipsWeightsDesc) == 15 * 8 + 6 * 4


def test_library_refuses_bad_arguments_without_launching():
    lib = _native.load()
    p = ctypes.c_void_p(256)                    # never dereferenced: every call below is refused before a launch
    desc = _native.LpipsWeightsDesc()
    for i in range(5):
        desc.conv_w[i] = desc.conv_b[i] = desc.lin[i] = 256
    w = ctypes.byref(desc)
    assert lib.virnet_lpips_workspace_bytes(2, 1, 31, 31) > 0
    assert lib.virnet_lpips_workspace_bytes(2, 1, 30, 31) == 0 and b"31x31" in lib.virnet_last_error()
    assert lib.virnet_lpips_workspace_bytes(2, 1, 31, 30) == 0 and b"31x31" in lib.virnet_last_error()
    assert lib.virnet_lpips_workspace_bytes(0, 0, 31, 31) == 0
    assert lib.virnet_lpips_workspace_bytes(2, 1, 20000, 20000) == 0 and b"2^31" in lib.virnet_last_error()
    assert lib.virnet_lpips(p, 0, p, 0, 1, 30, 40, w, p, p, None) != 0 and b"31x31" in lib.virnet_last_error()
    assert lib.virnet_lpips(p, 0, p, 0, 0, 40, 40, w, p, p, None) != 0 and b"batch" in lib.virnet_last_error()
    assert lib.virnet_lpips(None, 0, p, 0, 1, 40, 40, w, p, p, None) != 0 and b"NULL" in lib.virnet_last_error()
    assert lib.virnet_lpips(p, 0, p, 0, 1, 40, 40, None, p, p, None) != 0 and b"NULL" in lib.virnet_last_error()
    assert lib.virnet_lpips(p, 0, p, 0, 1, 40, 40, w, None, p, None) != 0 and b"NULL" in lib.virnet_last_error()
    assert lib.virnet_lpips(p, 0, p, 0, 1, 40, 40, w, ctypes.c_void_p(264), p, None) != 0 and b"aligned" in lib.virnet_last_error()
    assert lib.virnet_lpips(ctypes.c_void_p(258), 1, p, 0, 1, 40, 40, w, p, p, None) != 0 and b"misaligned" in lib.virnet_last_error()
    assert lib.virnet_lpips_features(p, 0, 1, 40, 30, w, p, p, p, p, p, p, None) != 0 and b"31x31" in lib.virnet_last_error()
    assert lib.virnet_lpips_features(p, 0, 1, 40, 40, w, p, p, p, None, p, p, None) != 0 and b"NULL" in lib.virnet_last_error()
    desc.lin[3] = None
    assert lib.virnet_lpips(p, 0, p, 0, 1, 40, 40, w, p, p, None) != 0 and b"stage 4" in lib.virnet_last_error()


def test_workspace_grows_with_the_maps_it_holds():
    lib = _native.load()
    sizes = lpips.map_sizes(97, 81)
    assert sizes == [(23, 19), (11, 9), (5, 4), (5, 4), (5, 4)]
    floats = 2 * (23 * 19 * 64 + 11 * 9 * 64 + 11 * 9 * 192 + 5 * 4 * (192 + 384 + 256 + 256))
    got = lib.virnet_lpips_workspace_bytes(2, 1, 97, 81)
    blocks = -(-23 * 19 // 64) + -(-11 * 9 // 64) + 3
    assert floats * 4 + blocks * 8 <= got <= floats * 4 + 7 * 256 + blocks * 8


# ---- weights --------------------------------------------------------------------------------------------------------------------------------
def _layout_a(w, lins="lin{}.model.1.weight", scaling=True):
    names = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
    sd = {}
    for i, n in enumerate(names):
        sd[n + ".weight"], sd[n + ".bias"] = w.conv_w[i].clone(), w.conv_b[i].clone()
        sd[lins.format(i)] = w.lin[i].clone().view(1, -1, 1, 1)
    if scaling:
        sd["scaling_layer.shift"], sd["scaling_layer.scale"] = w.shift.view(1, 3, 1, 1).clone(), w.scale.view(1, 3, 1, 1).clone()
    return sd


def _equal(x, y):
    return all(torch.equal(a, b) for a, b in zip(x.tensors().values(), y.tensors().values())) and list(x.tensors()) == list(y.tensors())


def test_load_weights_reads_both_layouts_and_the_module_prefix(tmp_path):
    w = lc.weights()
    assert _equal(lpips.load_weights(w.tensors()), w)
    assert _equal(lpips.load_weights(_layout_a(w)), w)
    assert _equal(lpips.load_weights(_layout_a(w, lins="lins.{}.model.1.weight", scaling=False)), w)       # constants when shift / scale are absent
    assert _equal(lpips.load_weights({"module." + k: v for k, v in _layout_a(w).items()}), w)
    assert _equal(lpips.load_weights({"module." + k: v for k, v in w.tensors().items()}), w)
    path = tmp_path / "lpips_alex.pt"
    torch.save(_layout_a(w), path)
    assert _equal(lpips.load_weights(str(path)), w)
    assert [float(v) for v in w.shift] == [np.float32(v) for v in (-0.030, -0.088, -0.188)]
    assert [float(v) for v in w.scale] == [np.float32(v) for v in (0.458, 0.448, 0.450)]
    assert [tuple(t.shape) for t in w.conv_w] == [(64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3)]
    assert all(float(v.min()) >= 0.0 for v in w.lin)
    assert _equal(lpips.synth_weights(lc.SEED), w) and not _equal(lpips.synth_weights(lc.SEED + 1), w)


def test_load_weights_refuses_by_name():
    w = lc.weights()
    sd = _layout_a(w)
    del sd["net.slice3.6.bias"]
    with pytest.raises(KeyError) as e:
        lpips.load_weights(sd)
    assert "conv3.bias" in str(e.value) and "net.slice3.6.bias" in str(e.value) and "net.slice3.6.weight" in str(e.value)   # looked for / found
    sd = w.tensors()
    del sd["lin4"]
    with pytest.raises(KeyError, match=r"lin4.*lin3\.model\.1\.weight.*lins\.3\.model\.1\.weight"):
        lpips.load_weights(sd)
    sd = w.tensors()
    sd["conv2.weight"] = sd["conv2.weight"][:, :, :3, :3]
    with pytest.raises(ValueError, match=r"conv2\.weight has shape \(192, 64, 3, 3\), \(192, 64, 5, 5\) expected"):
        lpips.load_weights(sd)
    sd = _layout_a(w)
    sd["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match="lin2 has shape"):
        lpips.load_weights(sd)
    sd = w.tensors()
    sd["shift"] = torch.zeros(4)
    with pytest.raises(ValueError, match="shift has shape"):
        lpips.load_weights(sd)
    with pytest.raises(TypeError, match="LpipsWeights"):
        lpips.distance_torch(*lc.pair_u8(lc.CASES[0]), w.tensors())


def test_weights_survive_deepcopy_and_torch_save():
    w = lc.weights()
    w._packed[torch.device("cuda", 0)] = {"stand-in": torch.zeros(1)}       # as after a device call
    try:
        c = copy.deepcopy(w)
        buf = io.BytesIO()
        torch.save(w, buf)
        buf.seek(0)
        r = torch.load(buf, weights_only=False)
    finally:
        w.drop_device_copies()
    assert _equal(c, w) and _equal(r, w) and c._packed == {} and r._packed == {}
    assert c.conv_w[0].data_ptr() != w.conv_w[0].data_ptr()
    assert not any(isinstance(v, (ctypes.Structure, ctypes._SimpleCData)) for v in vars(w).values())


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------
def _conv_np(x, wt, bias, stride, pad):
    """x [C,H,W] fp64, zero padding -> relu(conv) [Co,Ho,Wo]"""
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad)))
    k = wt.shape[-1]
    win = sliding_window_view(xp, (k, k), axis=(1, 2))[:, ::stride, ::stride]            # [C,Ho,Wo,k,k]
    return np.maximum(np.einsum("chwyx,ocyx->ohw", win, wt, optimize=False) + bias[:, None, None], 0.0)


def _pool_np(x):
    c, h, w = x.shape
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    out = np.empty((c, ho, wo))
    for y in range(ho):
        for xx in range(wo):
            out[:, y, xx] = x[:, 2 * y:2 * y + 3, 2 * xx:2 * xx + 3].max(axis=(1, 2))
    return out


def _quantise_np(x):
    if x.dtype == np.uint8:
        return x.astype(np.float64)
    x = np.where(np.isnan(x), np.float32(0), x)
    return np.rint(np.clip(x, np.float32(0), np.float32(1)).astype(np.float64) * 255.0)


def _taps_np(img, w, pad_before_scaling=False):
    """The five taps of one image [3,H,W] (uint8 or float32) in fp64, restated without torch."""
    x = (_quantise_np(img) - 127.5) / 127.5
    shift, scale = w.shift.numpy().astype(np.float64)[:, None, None], w.scale.numpy().astype(np.float64)[:, None, None]
    if pad_before_scaling:                              # the trap: a padded tap would then contribute (0 - shift) / scale
        x = (np.pad(x, ((0, 0), (2, 2), (2, 2))) - shift) / scale
    else:
        x = (x - shift) / scale
    taps = []
    for i, (_, _, _, stride, pad) in enumerate(lpips.CONVS):
        if i in (1, 2):
            x = _pool_np(x)
        x = _conv_np(x, w.conv_w[i].numpy().astype(np.float64), w.conv_b[i].numpy().astype(np.float64), stride,
                     0 if (i == 0 and pad_before_scaling) else pad)
        taps.append(x)
    return taps


def _distance_np(a, b, w):
    total = 0.0
    for fa, fb, lin in zip(_taps_np(a, w), _taps_np(b, w), w.lin):
        na = fa / (np.sqrt((fa ** 2).sum(0, keepdims=True)) + 1e-10)
        nb = fb / (np.sqrt((fb ** 2).sum(0, keepdims=True)) + 1e-10)
        total += ((na - nb) ** 2 * lin.numpy().astype(np.float64)[:, None, None]).sum(0).mean()
    return total


@pytest.mark.parametrize("form", lc.FORMS)
@pytest.mark.parametrize("case", lc.CASES[:2], ids=lc.IDS[:2])
def test_torch_definition_equals_the_numpy_restatement_in_fp64(case, form):
    w = lc.weights()
    a, b = lc.pair(case, form)
    d64, taps64 = lc.reference(case, form)
    assert d64.dtype == torch.float64 and [t.dtype for t in taps64] == [torch.float64] * 5
    assert [tuple(t.shape[1:]) for t in taps64] == [(c,) + s for c, s in zip(lpips.CHANNELS, lpips.map_sizes(*case[:2]))]
    want = _taps_np(a[0].numpy(), w)
    for i, (got, ref) in enumerate(zip(taps64, want)):
        err = np.abs(got[0].numpy() - ref).max() / np.abs(ref).max()
        print(f"tap {i + 1}: max-abs error / max {err:.3e}")
        assert err <= FP64_REL, i
    dn = _distance_np(a[0].numpy(), b[0].numpy(), w)
    rel = abs(float(d64[0]) - dn) / dn
    print(f"distance {dn:.9f} rel {rel:.3e}")
    assert 0.01 < dn < 1.0 and rel <= FP64_REL
    # conv1's border is where the padding rule shows: padding before the scaling layer moves the outermost outputs and no others
    wrong = _taps_np(a[0].numpy(), w, pad_before_scaling=True)[0]
    assert wrong.shape == want[0].shape
    assert np.abs(wrong[:, 0, :] - want[0][:, 0, :]).max() > 1e-3 and np.abs(wrong[:, :, 0] - want[0][:, :, 0]).max() > 1e-3
    np.testing.assert_allclose(wrong[:, 1:-1, 1:-1], want[0][:, 1:-1, 1:-1], rtol=0, atol=1e-12)
    if case == lc.CASES[1]:                   # 35 rows: the last window's bottom row is padding, so the last output row moves too
        assert np.abs(wrong[:, -1, 1:-1] - want[0][:, -1, 1:-1]).max() > 1e-3


def test_float_inputs_are_quantised_by_the_tables_rule():
    x, _ = lc.pair_f32(lc.CASES[0])
    assert bool(torch.isnan(x).any()) and float(x[~torch.isnan(x)].min()) < 0 and float(x[~torch.isnan(x)].max()) > 1
    q = lpips.quantise_torch(x)
    assert q.dtype == torch.float64 and float(q.min()) == 0.0 and float(q.max()) == 255.0 and not bool(torch.isnan(q).any())
    ref = veval.img_as_ubyte(np.clip(np.nan_to_num(x.numpy(), nan=0.0), 0.0, 1.0))
    np.testing.assert_array_equal(q.numpy().astype(np.uint8), ref)
    np.testing.assert_array_equal(q.numpy(), _quantise_np(x.numpy()))
    u = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16)
    assert torch.equal(lpips.quantise_torch(u.float() / 255.0), u.double())
    w = lc.weights()
    a, b = lc.pair_u8(lc.CASES[0])
    assert torch.equal(lpips.distance_torch(a.float() / 255.0, b, w, torch.float64), lc.reference(lc.CASES[0], "u8")[0])


def test_definition_is_zero_on_equal_images_symmetric_and_batch_independent():
    w = lc.weights()
    case = lc.CASES[2]
    a, b = lc.pair_u8(case)
    for dtype in (torch.float32, torch.float64):
        assert torch.equal(lpips.distance_torch(a, a.clone(), w, dtype), torch.zeros(2, dtype=dtype))
    d = lc.reference(case, "u8")[0]
    assert torch.equal(lpips.distance_torch(b, a, w, torch.float64), d)                   # (x - y)^2 == (y - x)^2 term by term
    for i in range(2):
        alone = lpips.distance_torch(a[i:i + 1], b[i:i + 1], w, torch.float64)
        assert abs(float(alone[0]) - float(d[i])) <= FP64_REL * float(d[i])
    assert float(d[0]) != float(d[1])


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_that_need_no_device():
    w = lc.weights()
    u8 = torch.zeros(1, 3, 31, 31, dtype=torch.uint8)
    for f in (lpips.distance, lpips.distance_torch):
        with pytest.raises(ValueError, match=r"\[N,3,H,W\]"):
            f(u8[0], u8[0], w)
        with pytest.raises(TypeError, match="uint8 or float32"):
            f(u8.double(), u8, w)
        with pytest.raises(TypeError, match="uint8 or float32"):
            f(u8, u8.half(), w)
        with pytest.raises(ValueError, match="same dimensions"):
            f(u8, torch.zeros(1, 3, 31, 32, dtype=torch.uint8), w)
        with pytest.raises(ValueError, match="channels"):
            f(u8[:, :1], u8[:, :1], w)
        with pytest.raises(ValueError, match="empty batch"):
            f(u8[:0], u8[:0], w)
        with pytest.raises(ValueError, match="at least 31x31"):
            f(u8[:, :, :30], u8[:, :, :30], w)
        with pytest.raises(ValueError, match="at least 31x31"):
            f(u8[:, :, :, :30], u8[:, :, :, :30], w)
        with pytest.raises(TypeError, match="LpipsWeights"):
            f(u8, u8, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lpips.distance(u8, u8, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lpips.features(u8, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.prepare("cpu")
    with pytest.raises(ValueError, match=r"2\^31"):
        lpips._check_size(2, 20000, 20000)
    with pytest.raises(ValueError, match=r"2\^31"):
        lpips._check_size(60000, 200, 200)
    lpips._check_size(2, 480, 320)
    with pytest.raises(TypeError, match="CUDA tensor"):
        lpips.table_pair(np.zeros((3, 31, 31), np.float32), np.zeros((31, 31, 3), np.uint8), w)
    with pytest.raises(RuntimeError, match="CUDA"):
        lpips.table_pair(torch.zeros(3, 31, 31), np.zeros((31, 31, 3), np.uint8), w)
    assert lpips.table_collect([]) == []


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def _two_bmps(tmp_path):
    from PIL import Image
    dst = tmp_path / "synth"
    dst.mkdir()
    files = []
    for i, case in enumerate(((66, 80, 1), (71, 65, 1))):                 # 71 x 65 is mod-cropped to 70 x 64 at sf 2
        im = lc.pair_u8(case)[0][0].numpy().transpose(1, 2, 0)
        files.append(str(dst / f"im{i}.bmp"))
        Image.fromarray(np.ascontiguousarray(im)).save(files[-1])
    return str(dst), files


def test_sisr_table_adds_the_lpips_keys_last(tmp_path):
    folder, files = _two_bmps(tmp_path)
    w = lc.weights()
    sf = 2
    kernels = sisr_eval.test_kernels(sf)[:2]

    def forward(lr, sf_):
        return np.repeat(np.repeat(lr, sf_, axis=0), sf_, axis=1) * np.float32(1.1) - np.float32(0.05)

    plain = sisr_eval.sisr_table(forward, [folder + ":bmp"], sf, kernels=kernels)
    assert plain == sisr_eval.sisr_table(forward, [folder + ":bmp"], sf, kernels=kernels, lpips=None)
    rows = sisr_eval.sisr_table(forward, [folder + ":bmp"], sf, kernels=kernels, lpips=w)
    assert len(rows) == len(plain) == 2
    for row, base, kernel in zip(rows, plain, kernels):
        assert list(base) == ["dataset", "kernel", "psnr_y", "ssim_y", "images", "per_image_psnr_y"]
        assert list(row) == list(base) + ["lpips", "per_image_lpips"]
        assert {k: row[k] for k in base} == base
        want = []
        for f in files:
            gt = sisr_eval.modcrop(veval.imread_rgb_uint8(f), sf)
            sr = veval.img_as_ubyte(np.clip(forward(sisr_eval.degrade(veval.img_as_float32(gt), kernel, sf), sf), 0.0, 1.0))
            assert sr.shape == gt.shape and gt.shape[0] % 2 == 0
            ta, tb = (torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[None])) for im in (sr, gt))
            want.append(float(lpips.distance_torch(ta, tb, w)[0]))
        assert row["per_image_lpips"] == want and row["lpips"] == float(np.mean(want))
        assert all(type(v) is float and 0.0 < v < 2.0 for v in want)
    with pytest.raises(TypeError, match="LpipsWeights"):
        sisr_eval.sisr_table(forward, [folder + ":bmp"], sf, kernels=kernels, lpips=w.tensors())
