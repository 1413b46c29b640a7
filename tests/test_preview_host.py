"""The host side of the training previews (virnet_amd/preview.py): ``grid_np`` against cases worked out by hand (torchvision is not
installed where the suite runs, so there is no golden for it), ``kernel_np`` against the reference's own ``util_sisr.kinfo2sigma`` fed
float64 (tests/golden/preview.npz, written by tests/golden/make_preview_golden.py), ``FolderWriter``, and the C ABI's new symbols."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from virnet_amd import _native
from virnet_amd import preview as pv

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
NEW_SYMBOLS = ("virnet_preview_grid_workspace_bytes", "virnet_preview_grid", "virnet_kernel_from_kinfo")


# ---- grid_np -----------------------------------------------------------------------------------------------------------------------------------
def test_one_image_is_its_own_grid_without_a_border():
    x = np.arange(3 * 5 * 7, dtype=F).reshape(1, 3, 5, 7)
    g = pv.grid_np(x)
    assert g.shape == (5, 7, 3) and g.dtype == np.uint8
    assert g[0, 0, 0] == 0 and g[4, 6, 2] == 255                                   # the minimum and the maximum of the image, at its corners
    assert np.array_equal(g, pv.grid_np(x, nrow=1, padding=9))                      # nrow and padding do not reach a single image
    assert pv.grid_shape(1, 5, 7) == (5, 7, 1, 1)


def test_nine_images_make_two_rows_with_seven_empty_cells():
    x = np.stack([np.full((3, 5, 7), 0.25, F) for _ in range(9)])
    x[:, :, 0, 0] = 0.0
    x[:, :, 4, 6] = 1.0                                                             # every image: 0 -> 0, 0.25 -> trunc(63.75) = 63, 1 -> 255
    g = pv.grid_np(x)
    assert pv.grid_shape(9, 5, 7) == (2 * 7 + 2, 8 * 9 + 2, 8, 2) and g.shape == (16, 74, 3)
    want = np.zeros((16, 74, 3), np.uint8)
    cell = np.full((5, 7, 3), 63, np.uint8)
    cell[0, 0], cell[4, 6] = 0, 255
    for k in range(9):
        y0, x0 = (k // 8) * 7 + 2, (k % 8) * 9 + 2
        want[y0:y0 + 5, x0:x0 + 7] = cell
    assert np.array_equal(g, want)
    assert not g[9:, 11:].any() and g[9:14, 2:9].any()                              # the second row: one image, seven empty cells, all zero
    assert not g[:2].any() and not g[:, :2].any() and not g[14:].any() and not g[:, 72:].any() and not g[7:9].any() and not g[:, 9:11].any()
    # other nrow / padding: the same cells elsewhere
    g4 = pv.grid_np(x, nrow=4, padding=1)
    assert g4.shape == (3 * 6 + 1, 4 * 8 + 1, 3) and np.array_equal(g4[13:18, 1:8], cell) and not g4[13:18, 8:].any()
    g0 = pv.grid_np(x[:2], padding=0)
    assert g0.shape == (5, 14, 3) and np.array_equal(g0[:, 7:], cell)


def test_a_single_plane_goes_to_all_three_channels():
    x = np.random.default_rng(0).random((3, 1, 6, 5), dtype=F)
    g = pv.grid_np(x)
    assert g.shape == (8 + 2, 3 * 7 + 2, 3)
    assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 0], g[..., 2]) and g.max() == 255
    rgb = pv.grid_np(np.repeat(x, 3, axis=1))
    assert np.array_equal(g, rgb)


def test_a_constant_image_divides_by_1e_5_and_is_all_zeros():
    x = np.full((2, 3, 4, 4), 0.7, F)
    x[1, 0, 0, 0] = F(0.7) + F(2e-6)                     # range 2e-6 (a few ulps) < 1e-5: the divisor is 1e-5, the maximum maps to about 0.2 * 255
    g = pv.grid_np(x)
    assert not g[2:6, 2:6].any()
    d = F(1e-5)
    top = int(F(F(x[1, 0, 0, 0] - F(0.7)) / d) * F(255))
    assert 40 <= top <= 60 and g[2, 8, 0] == top and g[2:6, 8:12].sum() == top


def test_quantisation_truncates():
    # lo = 0, hi = 1, d = 1: y = x.  255 -> 255 exactly; 100 / 255 rounded to float32 times 255 lands just below or on 100
    vals = np.array([0.0, 1.0, 0.5, 100.0 / 255.0, np.nextafter(F(100.0 / 255.0), F(0)), 0.999999, 1.0 / 255.0 - 1e-6, 254.5 / 255.0], dtype=F)
    x = vals.reshape(1, 1, 1, -1)
    g = pv.grid_np(x)[0, :, 0]
    assert g[0] == 0 and g[1] == 255 and g[2] == 127                                # 127.5 truncates, it does not round
    exact = [int(np.floor(float(F(v * F(255))))) for v in vals]                     # float32 product, then floor: the definition's own steps
    assert g.tolist() == exact
    assert g[4] == 99 and g[5] == 254 and g[6] == 0 and g[7] == 254                 # just below a boundary: one lower
    # a scaled image: the maximum maps to exactly 255 whatever the range
    y = (vals * F(37.5) - F(11.0)).reshape(1, 1, 1, -1)
    gy = pv.grid_np(y)[0, :, 0]
    assert gy[1] == 255 and gy[0] == 0


def test_negative_inputs_and_the_clamp_on_load():
    x = np.array([-2.0, -1.0, 0.0, 0.5, 1.0, 3.0], dtype=F).reshape(1, 1, 2, 3)
    g = pv.grid_np(x)[..., 0].reshape(-1)
    assert g.tolist() == [0, 51, 102, 127, 153, 255]                                # (x + 2) / 5 * 255, truncated
    keep = x.copy()
    gc = pv.grid_np(x, clamp=(0.0, 1.0))[..., 0].reshape(-1)
    assert gc.tolist() == [0, 0, 0, 127, 255, 255] and np.array_equal(x, keep)      # clamped copy: [0, 0, 0, .5, 1, 1]; the input is not written
    assert np.array_equal(pv.grid_np(x, clamp=(0.0, 1.0)), pv.grid_np(np.clip(x, 0, 1)))


def test_non_finite_elements():
    x = np.zeros((3, 1, 2, 3), dtype=F)
    x[0, 0] = [[0.0, 1.0, np.nan], [np.inf, -np.inf, 0.5]]
    x[1, 0] = np.nan
    x[1, 0, 1, 1] = -np.inf
    x[1, 0, 0, 0] = np.inf                                                          # no finite element: all zeros, the +inf too
    x[2, 0] = [[2.0, 4.0, 3.0], [2.0, 2.0, 2.0]]
    g = pv.grid_np(x)[..., 0]
    assert g[2:4, 2:5].tolist() == [[0, 255, 0], [255, 0, 127]]                     # NaN and -inf: 0; +inf: 255; min / max from the finite ones
    assert not g[2:4, 7:10].any()
    assert g[2:4, 12:15].tolist() == [[0, 255, 127], [0, 0, 0]]                     # the neighbour is untouched
    clean = x.copy()
    clean[0, 0] = [[0.0, 1.0, 0.0], [1.0, 0.0, 0.5]]
    clean[1] = 0
    assert np.array_equal(pv.grid_np(x), pv.grid_np(clean))
    # under a clamp the infinities are finite before the range is taken
    gc = pv.grid_np(x[:1], clamp=(0.0, 1.0))[..., 0]
    assert gc.tolist() == [[0, 255, 0], [255, 0, 127]]


def test_grid_np_refuses_what_it_does_not_define():
    with pytest.raises(TypeError):
        pv.grid_np(np.zeros((1, 2, 4, 4), F))
    with pytest.raises(TypeError):
        pv.grid_np(np.zeros((1, 3, 4, 4), np.float64))
    with pytest.raises(ValueError):
        pv.grid_np(np.zeros((1, 3, 4, 4), F), nrow=0)


# ---- kernel_np ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "preview.npz"))


def test_golden_inputs_are_well_conditioned_and_the_reference_agrees_with_itself(golden):
    """The bar of the next test, 1e-12 absolute, is fixed only after this: on these inputs the reference evaluated on the whole batch and on
    every sample alone (last first) gives the same fp64 values to 1e-12."""
    cases, kinfo = golden["cases"], golden["kinfo"]
    assert sorted({int(k) for k, _, _ in cases}) == [15, 21] and sorted({int(sf) for _, sf, _ in cases}) == [2, 3, 4]
    assert {int(s) for _, _, s in cases} == {0, 1} and kinfo.dtype == np.float32
    for (k, sf, _), info in zip(cases, kinfo):
        assert (info[:, :2] >= 0.5).all() and (info[:, :2] <= 3.0 * sf * sf).all() and (np.abs(info[:, 2]) <= 0.9 + 1e-7).all()
    assert np.abs(golden["kernel"] - golden["kernel_alone"]).max() <= 1e-12


def test_kernel_np_is_the_references_kinfo2sigma(golden):
    for (k, sf, shift), info, want in zip(golden["cases"], golden["kinfo"], golden["kernel"]):
        k = int(k)
        got = pv.kernel_f64_np(info, k, int(sf), bool(shift))
        assert got.shape == (len(info), 1, k, k) and got.dtype == np.float64
        assert np.abs(got[:, 0] - want[:, :k, :k]).max() <= 1e-12, (k, sf, shift)
        got32 = pv.kernel_np(info, k, int(sf), bool(shift))
        assert got32.dtype == np.float32 and np.array_equal(got32, got.astype(np.float32))
        assert np.abs(got32.astype(np.float64).sum(axis=(1, 2, 3)) - 1.0).max() <= 1e-6


def test_the_shift_moves_the_centre(golden):
    info = golden["kinfo"][0][:1]
    plain, moved = pv.kernel_np(info, 21, 2, False)[0, 0], pv.kernel_np(info, 21, 2, True)[0, 0]
    assert np.unravel_index(plain.argmax(), plain.shape) == (10, 10) and pv.kernel_centre(21, 2, True) == 10.5 and pv.kernel_centre(15, 4, True) == 8.5
    assert plain[10, 10] > plain[11, 11] and abs(moved[10, 10] - moved[11, 11]) < 1e-7 * moved.max()


def test_a_singular_sample_gets_1e_5_on_its_own_diagonal(golden):
    info = golden["singular_kinfo"]
    assert info.tolist() == [[1.0, 1.0, 1.0]]
    got = pv.kernel_f64_np(info, 21, 2, False)
    assert np.isfinite(got).all() and np.abs(got[:, 0] - golden["singular_kernel"]).max() <= 1e-12
    # inside a batch the nudge stays with that sample: its neighbours are what they are alone
    batch = np.concatenate([golden["kinfo"][0][:2], info, golden["kinfo"][0][2:3]])
    both = pv.kernel_f64_np(batch, 21, 2, False)
    assert np.array_equal(both[2], got[0]) and np.array_equal(both[[0, 1, 3]], pv.kernel_f64_np(golden["kinfo"][0][:3], 21, 2, False))


# ---- FolderWriter ------------------------------------------------------------------------------------------------------------------------------
def test_folder_writer_round_trip(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    im = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    with pv.FolderWriter(tmp_path / "run") as w:
        w.add_scalar("Train Loss Iter", np.float32(1.5), 0)
        w.add_image("train Denoised images", im, 7, dataformats="HWC")
        w.add_scalar("PSNR_epoch_test", 30.25, 3)
        with pytest.raises(TypeError):
            w.add_image("x", im.astype(np.float32), 0)
        with pytest.raises(TypeError):
            w.add_image("x", im.transpose(2, 0, 1), 0, dataformats="CHW")
    path = tmp_path / "run" / "images" / "train_Denoised_images" / "000007.png"
    assert path.exists() and np.array_equal(np.asarray(Image.open(path)), im)
    lines = [json.loads(line) for line in open(tmp_path / "run" / "scalars.jsonl")]
    assert lines == [{"tag": "Train Loss Iter", "value": 1.5, "step": 0}, {"tag": "PSNR_epoch_test", "value": 30.25, "step": 3}]
    w.close()                                                                       # a second close is harmless
    with pv.FolderWriter(tmp_path / "run") as again:                                # a resumed run appends
        again.add_scalar("Loss_epoch", 2.0, 1)
    assert len(open(tmp_path / "run" / "scalars.jsonl").readlines()) == 3


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    with open(_native.HEADER_PATH) as f:
        text = f.read()
    assert "#define VIRNET_ABI_VERSION 5" in text and _native.ABI_VERSION == 5
    declared = {name: (restype, argtypes) for name, restype, argtypes in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in declared, name
    assert len(declared["virnet_preview_grid"][1]) == 16 and len(declared["virnet_kernel_from_kinfo"][1]) == 7
    lib = _native.load()
    assert lib.virnet_abi_version() == 5
    assert lib.virnet_preview_grid_workspace_bytes(32) == 32 * 2 * 4 and lib.virnet_preview_grid_workspace_bytes(0) == 0
    # the header's declarations equal the library's exports
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (virnet_\w+)", out))
    assert exported == set(declared), (sorted(exported - set(declared)), sorted(set(declared) - exported))


def test_bad_arguments_are_refused_on_the_host():
    lib = _native.load()
    big = 1 << 16
    # (pointers are checked first, so a refused call never launches; 16 stands in for a non-NULL address)
    for args, word in [((16, 3 * 4 * 4, 2, 2, 4, 4, 8, 2, 0, 0.0, 0.0, 16, 16, 14, 14, None), "channels"),
                       ((16, 3 * 4 * 4, 2, 3, 4, 4, 8, 2, 0, 0.0, 0.0, 16, 16, 9, 14, None), "the output is"),
                       ((16, 3 * big * big, 2, 3, big, big, 8, 2, 0, 0.0, 0.0, 16, 16, 1, 1, None), "2^31"),
                       ((16, 3 * 4 * 4, 1 << 20, 3, 4, 4, 1 << 20, 2000, 0, 0.0, 0.0, 16, 16, 1, 1, None), "2^31"),
                       ((16, 10, 2, 3, 4, 4, 8, 2, 0, 0.0, 0.0, 16, 16, 8, 14, None), "batch stride"),
                       ((16, 48, 2, 3, 4, 4, 8, 2, 1, 1.0, 0.0, 16, 16, 8, 14, None), "clamp"),
                       ((0, 48, 2, 3, 4, 4, 8, 2, 0, 0.0, 0.0, 16, 16, 8, 14, None), "NULL")]:
        assert lib.virnet_preview_grid(*args) != 0
        assert word in lib.virnet_last_error().decode(), (word, lib.virnet_last_error())
    assert lib.virnet_kernel_from_kinfo(16, 2, 27, 2, 0, 16, None) != 0 and "1..25" in lib.virnet_last_error().decode()
    assert lib.virnet_kernel_from_kinfo(16, 0, 21, 2, 0, 16, None) != 0


# ---- the drivers' flag ---------------------------------------------------------------------------------------------------------------------------
def test_previews_flag_gives_a_folder_writer_on_rank_0(tmp_path, monkeypatch):
    import sys
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(HERE), "tools"))
    import train_common as tc
    assert tc.parse_flags([], "d.json", "./rec", "help").previews is None
    opts = tc.parse_flags(["--previews", str(tmp_path / "pv")], "d.json", "./rec", "help")
    assert opts.previews == str(tmp_path / "pv")
    assert tc.summary_writer({}) is None and not (tmp_path / "pv").exists()
    monkeypatch.setenv("RANK", "1")
    assert tc.summary_writer({"previews": opts.previews}) is None and not (tmp_path / "pv").exists()
    monkeypatch.setenv("RANK", "0")
    w = tc.summary_writer({"previews": opts.previews})
    assert isinstance(w, pv.FolderWriter) and (tmp_path / "pv" / "images").is_dir()
    w.close()
    for name in ("train_denoising_syn.py", "train_denoising_real.py", "train_sisr.py"):
        with open(os.path.join(os.path.dirname(HERE), "tools", name)) as f:
            assert "writer=tc.summary_writer(args)" in f.read(), name
    sys.modules.pop("train_common", None)
