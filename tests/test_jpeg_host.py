"""Host-side checks of the JPEG round trip (virnet_amd/jpeg.py, csrc/jpeg.hip): the integer definition reproduces Pillow's libjpeg-turbo
byte for byte on every fixture case and its tables at all 100 qualities, the host wiring (eval.jpeg_compress, sisr_eval.degrade(qf=),
sisr_eval.synthesize_lr_np) is what it says, the C ABI is bound at version 5, the kernels use no scratch, and argument errors are raised
before any device work."""
import numpy as np
import pytest
import torch

import jpeg_cases
from conftest import load_golden
from test_kernel_resources import _remarks, _table
from virnet_amd import _native, jpeg, sisr_eval
from virnet_amd import eval as veval

NEW_SYMBOLS = ("virnet_jpeg_workspace_bytes", "virnet_jpeg_roundtrip")


def test_fixture_holds_the_cases_it_should():
    f = jpeg_cases.fixture()
    assert set(jpeg_cases.sizes()) >= {(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (31, 16), (37, 51), (40, 56)}
    assert list(f["kinds"]) == ["uniform", "smooth", "saturated", "checker"] and list(f["qualities"]) == [1, 10, 40, 75, 95, 100]
    assert any("libjpeg-turbo" in str(v) for v in f["versions"]) and any("Pillow" in str(v) for v in f["versions"])
    sat = f["in_40x56_saturated"]
    assert set(np.unique(sat)) == {0, 255}
    chk = f["in_7x9_checker"][:, :, 0]
    assert (chk[:, 1:] != chk[:, :-1]).all() and (chk[1:] != chk[:-1]).all()


@pytest.mark.parametrize("h,w", jpeg_cases.sizes())
def test_roundtrip_np_equals_libjpeg_byte_for_byte(h, w):
    for kind, q, im, want in jpeg_cases.cases(h, w):
        got = jpeg.roundtrip_np(im, q)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert int((got != want).sum()) == 0, (h, w, kind, q, int((got != want).sum()))


def test_quant_tables_equal_libjpeg_at_every_quality():
    tables = jpeg_cases.fixture()["tables"]
    both = jpeg.all_quant_tables()
    assert both.dtype == np.int32 and both.shape == (101, 2, 64) and not both[0].any()
    for q in range(1, 101):
        luma, chroma = jpeg.quant_tables(q)
        assert luma.dtype == np.int32 and luma.shape == (8, 8) and chroma.dtype == np.int32 and chroma.shape == (8, 8)
        assert np.array_equal(luma.reshape(-1), tables[q, 0]) and np.array_equal(chroma.reshape(-1), tables[q, 1]), q
        assert np.array_equal(both[q, 0], tables[q, 0]) and np.array_equal(both[q, 1], tables[q, 1])
    for q, same in ((0, 1), (-5, 1), (101, 100), (1000, 100)):                 # clipped to 1..100
        assert all(np.array_equal(a, b) for a, b in zip(jpeg.quant_tables(q), jpeg.quant_tables(same)))


def test_roundtrip_np_argument_errors():
    with pytest.raises(TypeError):
        jpeg.roundtrip_np(np.zeros((8, 8, 3), dtype=np.float32), 40)
    with pytest.raises(TypeError):
        jpeg.roundtrip_np(np.zeros((8, 8), dtype=np.uint8), 40)
    with pytest.raises(ValueError):
        jpeg.roundtrip_np(np.zeros((0, 8, 3), dtype=np.uint8), 40)


def test_eval_jpeg_compress_dtypes():
    g = np.random.default_rng(5)
    x = (g.random((17, 33, 3)) * 1.2 - 0.1).astype(np.float32)
    x[0, :8, 0] = (np.arange(8, dtype=np.float32) + np.float32(0.5)) / np.float32(255.0)
    got = veval.jpeg_compress(x, 40)
    assert got.dtype == np.float32
    assert np.array_equal(got, veval.img_as_float32(jpeg.roundtrip_np(veval.img_as_ubyte(x), 40)))
    u8 = veval.img_as_ubyte(x)
    got8 = veval.jpeg_compress(u8, 40)
    assert got8.dtype == np.uint8 and np.array_equal(got8, jpeg.roundtrip_np(u8, 40))
    got64 = veval.jpeg_compress(x.astype(np.float64), 40)
    assert got64.dtype == np.float64 and np.array_equal(got64, got.astype(np.float64))
    with pytest.raises(TypeError):
        veval.jpeg_compress(np.zeros((8, 8, 3), dtype=np.int32), 40)


@pytest.fixture(scope="module")
def small_image():
    g = np.random.default_rng(11)
    yy, xx = np.mgrid[0:48, 0:40]
    im = np.stack([0.5 + 0.4 * np.sin(0.2 * xx + 0.1 * yy), yy / 48.0, xx / 40.0], axis=-1) + g.normal(0.0, 0.05, (48, 40, 3))
    return np.clip(im, 0.0, 1.0).astype(np.float32), sisr_eval.test_kernels(2)[4]


@pytest.mark.parametrize("down", ["bicubic", "direct"])
def test_degrade_qf_default_is_unchanged_and_qf_is_the_round_trip(small_image, down):
    im, kernel = small_image
    plain = sisr_eval.degrade(im, kernel, 2, downsampler=down)
    assert np.array_equal(sisr_eval.degrade(im, kernel, 2, downsampler=down, qf=None), plain)
    got = sisr_eval.degrade(im, kernel, 2, downsampler=down, qf=40)
    assert got.dtype == np.float32 and np.array_equal(got, veval.jpeg_compress(plain, 40))
    assert not np.array_equal(got, plain)


def test_degrade_default_still_matches_the_reference_golden():
    """the pinned output of the reference's degrade_virnet (qf=None) is reproduced as before: the new argument changes nothing by default"""
    G = load_golden("sisr_harness")
    gt = veval.imread_rgb_uint8(jpeg_cases.GOLDEN + "/set5/butterfly_GT.bmp")
    im = veval.img_as_float32(sisr_eval.modcrop(gt, 2))
    got = sisr_eval.degrade(im, G["kernels_sf2"][6], 2, downsampler="direct")
    assert np.array_equal(got, sisr_eval.degrade(im, G["kernels_sf2"][6], 2, downsampler="direct", qf=None))
    assert np.abs(got - G["lr_sf2_k6_direct"]).max() <= 1e-6


@pytest.mark.parametrize("down", ["bicubic", "direct"])
def test_synthesize_lr_np_is_blur_noise_clip_round_trip(small_image, down):
    im, kernel = small_image
    g = np.random.default_rng(3)
    noise = g.standard_normal((24, 20, 3)).astype(np.float32)
    std = 7.0 / 255.0
    lr0, blur = sisr_eval.synthesize_lr_np(im, kernel, 2, noise, std, 0, down)
    assert lr0.dtype == np.float32 and blur.dtype == np.float32 and lr0.shape == blur.shape == (24, 20, 3)
    # the blur is sisr_eval.degrade's without its noise (nlevel 0), up to that function's float64 sum for the bicubic resize
    assert np.abs(blur - sisr_eval.degrade(im, kernel, 2, nlevel=0.0, downsampler=down)).max() <= 2.0 ** -23
    want = np.clip(blur + noise * np.float32(std), np.float32(0), np.float32(1))
    assert np.array_equal(lr0, want) and np.array_equal(lr0, sisr_eval.synthesize_tail_np(blur, noise, std, 0))
    lr30, blur30 = sisr_eval.synthesize_lr_np(im, kernel, 2, noise, std, 30, down)
    assert np.array_equal(blur30, blur) and np.array_equal(lr30, veval.jpeg_compress(want, 30))


def test_new_symbols_bound_and_abi_version_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5


def test_jpeg_kernels_use_no_scratch():
    """the compiler's own resource remarks, as tests/test_kernel_resources.py reads them: zero scratch, no spilled vector register"""
    rows = _table(_remarks("jpeg"))
    assert {r["pretty"] for r in rows} == {"jpeg_blocks_kernel", "jpeg_finish_kernel"}
    for r in rows:
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r


def test_c_abi_argument_errors_return_nonzero_with_a_message():
    """bad sizes never reach a launch (no device needed, the pointers are never read)"""
    lib = _native.load()
    p = 4096
    assert lib.virnet_jpeg_workspace_bytes(2, 37, 51) == 2 * (37 * 51 + 2 * 19 * 26)
    assert lib.virnet_jpeg_workspace_bytes(1, 1, 1) == 3 and lib.virnet_jpeg_workspace_bytes(32, 256, 256) == 32 * 256 * 256 * 3 // 2
    for n, h, w in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 32769, 8), (1, 8, 32769), (-1, 8, 8)):
        assert lib.virnet_jpeg_workspace_bytes(n, h, w) == 0
        assert lib.virnet_jpeg_roundtrip(p, 0, p, 0, p, p, p, n, h, w, None) != 0 and "outside" in lib.virnet_last_error().decode()
    for bad in range(5):
        ptrs = [p] * 5
        ptrs[bad] = 0
        assert lib.virnet_jpeg_roundtrip(ptrs[0], 1, ptrs[1], 1, ptrs[2], ptrs[3], ptrs[4], 1, 8, 8, None) != 0
        assert "NULL" in lib.virnet_last_error().decode()


class _NoLaunch:
    """stands in for the loaded library: any call into it is an error"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: argument errors must be raised before any device work")


@pytest.fixture
def no_device_work(monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: _NoLaunch())
    monkeypatch.setattr(jpeg, "_device_tables", lambda device: (_ for _ in ()).throw(AssertionError("the table upload was reached")))


@pytest.mark.parametrize("case, exc", [("not_tensor", TypeError), ("dtype", TypeError), ("dims", ValueError), ("channels", ValueError),
                                       ("empty", ValueError), ("qf_float", TypeError), ("qf_none", TypeError), ("qf_bool", TypeError),
                                       ("qf_101", ValueError), ("qf_negative", ValueError), ("qf_len", ValueError), ("qf_list_float", TypeError),
                                       ("qf_list_range", ValueError), ("qf_tensor_dtype", TypeError), ("qf_tensor_shape", ValueError),
                                       ("cpu", RuntimeError), ("cpu_list", RuntimeError), ("cpu_tensor_qf", RuntimeError)])
def test_argument_errors_before_device_work(no_device_work, case, exc):
    x, qf = torch.zeros(2, 3, 16, 16), 40
    if case == "not_tensor":
        x = np.zeros((2, 3, 16, 16), dtype=np.float32)
    elif case == "dtype":
        x = x.double()
    elif case == "dims":
        x = torch.zeros(3, 16, 16)
    elif case == "channels":
        x = torch.zeros(2, 1, 16, 16)
    elif case == "empty":
        x = torch.zeros(2, 3, 0, 16)
    elif case == "qf_float":
        qf = 40.0
    elif case == "qf_none":
        qf = None
    elif case == "qf_bool":
        qf = True
    elif case == "qf_101":
        qf = 101
    elif case == "qf_negative":
        qf = -1
    elif case == "qf_len":
        qf = [40, 40, 40]
    elif case == "qf_list_float":
        qf = [40, 40.5]
    elif case == "qf_list_range":
        qf = [40, 101]
    elif case == "qf_tensor_dtype":
        qf = torch.tensor([40, 40])
    elif case == "qf_tensor_shape":
        qf = torch.tensor([40, 40, 40], dtype=torch.int32)
    elif case == "cpu_list":
        qf = [40, 0]
    elif case == "cpu_tensor_qf":
        x, qf = x.to(torch.uint8), torch.tensor([40, 0], dtype=torch.int32)
    with pytest.raises(exc) as e:
        jpeg.jpeg_compress(x, qf)
    if exc is RuntimeError:
        assert "no CPU fallback" in str(e.value)


def test_wiring_argument_errors_before_the_device_check(no_device_work):
    from virnet_amd import degrade
    im, ker = np.zeros((32, 32, 3), dtype=np.float32), np.ones((21, 21)) / 441.0
    for bad in (0, 101, 40.5, True):
        with pytest.raises(ValueError):
            degrade.degrade_lr(im, ker, 2, qf=bad)
    x, k = torch.zeros(2, 3, 32, 32), torch.zeros(2, 1, 21, 21)
    noise, std = torch.zeros(2, 3, 16, 16), torch.zeros(2)
    with pytest.raises(ValueError):
        degrade.synthesize_lr(x, k, 2, torch.zeros(2, 3, 15, 16), std)
    with pytest.raises(ValueError):
        degrade.synthesize_lr(x, k, 2, noise, torch.zeros(3))
    with pytest.raises(TypeError):
        degrade.synthesize_lr(x, k, 2, noise.double(), std)
    with pytest.raises(ValueError):
        degrade.synthesize_lr(x, k, 5, noise, std)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        degrade.synthesize_lr(x, k, 2, noise, std, torch.zeros(2, dtype=torch.int32))
