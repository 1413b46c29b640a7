"""CPU tests of tiled whole-image restoration (virnet_amd/restore.py, csrc/restore.hip): the ABI, the kernels' resources, the plan's
tap tables against ``forward_tiled``'s stitching, ``auto_tile`` against the library's own 2 GB check, the host definitions' properties
and the argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import restore_cases as rc
from test_kernel_resources import _remarks, _table
from test_launch_plan import desc_of
from virnet_amd import _native, ops, restore
from virnet_amd.utils.tiling import forward_tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP1 = float(np.spacing(np.float32(1.0)))          # one fp32 ulp at 1.0


def test_symbols_are_exported_declared_and_bound_and_the_abi_is_5():
    lib = _native.load()
    assert lib.virnet_abi_version() == 5 == _native.ABI_VERSION
    with open(os.path.join(ROOT, "include", "virnet_hip.h")) as f:
        header = f.read()
    assert "#define VIRNET_ABI_VERSION 5" in header
    for name, nargs in (("virnet_tile_gather", 12), ("virnet_tile_blend", 24)):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
        decl = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M | re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert re.search(r"#define VIRNET_TILE_SLOTS %d\b" % restore.K, header) and re.search(r"#define VIRNET_TILE_BOXES %d\b" % restore.MAX_BOXES, header)
    boxes = (ctypes.c_int * 2)(0, 0)
    assert lib.virnet_tile_gather(None, 0, 0, 8, 8, 3, boxes, 1, 4, 4, None, None) != 0 and b"NULL" in lib.virnet_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.virnet_tile_gather(p, 0, 0, 8, 8, 5, boxes, 1, 4, 4, p, None) != 0 and b"5 channels" in lib.virnet_last_error()
    boxes = (ctypes.c_int * 2)(5, 0)
    assert lib.virnet_tile_gather(p, 0, 0, 8, 8, 3, boxes, 1, 4, 4, p, None) != 0 and b"(5, 0)" in lib.virnet_last_error()


def test_new_unit_uses_no_scratch():
    rows = _table(_remarks("restore"))
    assert len([r for r in rows if "tile_gather_kernel" in r["pretty"]]) == 2                 # uint8, fp32
    assert len([r for r in rows if "tile_blend_kernel" in r["pretty"]]) == 16                 # 2 types x 4 channel counts x 2 modes
    for r in rows:
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
GRID = [(H, W, tile, overlap, scale) for (tile, overlap) in ((16, 4), (32, 8)) for (H, W) in ((37, 53), (64, 100), (100, 37), (53, 64))
        for scale in (1, 2, 3)] + [(20, 100, 32, 8, 2)]                                       # the last: th = H < tile


@pytest.mark.parametrize("H,W,tile,overlap,scale", GRID)
def test_crop_plan_is_forward_tiled_ownership(H, W, tile, overlap, scale):
    p = restore.plan(H, W, tile, overlap, scale=scale, blend="crop")
    owner = rc.forward_tiled_index(H, W, tile, overlap, scale)
    assert owner.min() >= 0
    assert (p.row_idx[:, 1:] == -1).all() and (p.col_idx[:, 1:] == -1).all()
    assert (p.row_w[:, 0] == 1).all() and (p.col_w[:, 0] == 1).all()
    assert np.array_equal(p.row_idx[:, 0][:, None].astype(np.int64) * p.nx + p.col_idx[:, 0][None, :], owner)
    assert p.boxes == [(y, x) for y in p.ys for x in p.xs] and (p.th, p.tw) == (min(tile, H), min(tile, W))


@pytest.mark.parametrize("H,W,tile,overlap,scale", GRID)
def test_linear_plan_covers_every_position_with_weights_that_sum_to_one(H, W, tile, overlap, scale):
    p = restore.plan(H, W, tile, overlap, scale=scale, blend="linear")
    for idx, wgt, starts, t, size in ((p.row_idx, p.row_w, p.ys, p.th, H), (p.col_idx, p.col_w, p.xs, p.tw, W)):
        assert idx.shape == wgt.shape == (size * scale, restore.K) and idx.dtype == np.int32 and wgt.dtype == np.float32
        used = idx >= 0
        n = used.sum(axis=1)
        assert n.min() >= 1 and n.max() <= 3
        assert (used[:, :-1] >= used[:, 1:]).all()                                            # used slots first ...
        assert all((np.diff(row[row >= 0]) > 0).all() for row in idx)                         # ... in ascending tile order
        assert (wgt[used] > 0).all() and (wgt[~used] == 0).all()
        assert np.abs(wgt.astype(np.float64).sum(axis=1) - 1.0).max() <= ULP1
        assert (wgt[n == 1, 0] == 1.0).all()
        q = np.arange(size * scale)
        cover = np.stack([(q >= s * scale) & (q < (s + t) * scale) for s in starts])          # every covering tile has a slot, no other
        assert np.array_equal(cover.sum(axis=0), n)
        for k in range(restore.K):
            on = idx[:, k] >= 0
            assert cover[idx[on, k], q[on]].all()
        # the weights are the normalised ramps of the definition
        cap = 2 * overlap * scale
        raw = np.zeros(cover.shape)
        for i, s in enumerate(starts):
            L = q - s * scale + 1 if s != 0 else np.full(q.shape, cap)
            R = (s + t) * scale - q if s + t != size else np.full(q.shape, cap)
            raw[i] = np.where(cover[i], np.minimum(np.minimum(L, R), cap), 0)
        want = raw / raw.sum(axis=0)
        for k in range(restore.K):
            on = idx[:, k] >= 0
            assert np.array_equal(wgt[on, k], want[idx[on, k], q[on]].astype(np.float32))


def test_the_grid_has_a_three_way_overlap_and_a_short_axis():
    p = restore.plan(37, 53, 16, 4)
    assert p.ys == [0, 8, 16, 21] and (p.row_idx[21:24] >= 0).all()                           # rows 21..23 lie under tiles 1, 2 and 3
    short = restore.plan(20, 100, 32, 8, scale=2)
    assert (short.th, short.tw, short.ny) == (20, 32, 1) and (short.row_idx[:, 0] == 0).all() and (short.row_w[:, 0] == 1).all()


# ---- auto_tile and the library's limit ---------------------------------------------------------------------------------------------------
def _library_accepts(h, w, c):
    d = desc_of([_native.PLAN_WX4, 1, h, w, c, c, 1, 0, 1, 1, 0, 256])
    try:
        ops.conv_plan_query(_native.PLAN_WX4, d, n_cu=256)
        return True
    except RuntimeError as e:
        assert "below 2 GB" in str(e), e
        return False


def test_auto_tile_follows_the_library_check():
    tile = restore.auto_tile(3000, 4000, 96, 1)
    assert 0 < tile <= 1024 and tile % 4 == 0
    assert restore.fits(tile, tile, 96) and _library_accepts(tile, tile, 96) and not _library_accepts(3000, 4000, 96)
    assert restore.auto_tile(256, 256, 96, 1) == 0
    small = restore.auto_tile(96, 80, 96, 1, limit_bytes=2 ** 20)
    assert 0 < small < 80 and small % 4 == 0 and restore.fits(small, small, 96, 2 ** 20) and not restore.fits(small + 4, small + 4, 96, 2 ** 20)
    assert restore.auto_tile(96, 80, 96, 2, limit_bytes=2 ** 20) * 2 <= small + 4              # the output grid counts at scale 2
    with pytest.raises(ValueError, match="no tile"):
        restore.auto_tile(96, 80, 96, 1, limit_bytes=1000)
    # the boundary of the one formula: 96 channels, 2048 columns -> 2^31 bytes at exactly 2731 rows
    w, c = 2048, 96
    rows = (2 ** 31 - 1) // (w * c * 4)                                                       # the last count below the limit
    assert restore.fits(rows, w, c) and not restore.fits(rows + 1, w, c)
    assert _library_accepts(rows, w, c) and not _library_accepts(rows + 1, w, c)
    assert restore.auto_tile(rows, w, c, 1) == 0 and restore.auto_tile(rows + 1, w, c, 1) > 0


def test_widest_channels_come_from_the_module():
    from virnet_amd.networks import VIRAttResUNet, VIRAttResUNetSR
    den = VIRAttResUNet(im_chn=3, sigma_chn=1, n_feat=[96, 192, 288], dep_S=5, n_resblocks=3, noise_cond=True, extra_mode="Input", noise_avg=False)
    assert restore.widest_channels(den) == 96
    sr = VIRAttResUNetSR(im_chn=3, sigma_chn=1, kernel_chn=3, n_feat=[32, 160, 224], dep_S=5, dep_K=8, n_resblocks=2, extra_mode="Both")
    assert restore.widest_channels(sr) == 64                                                  # SNet's 64 filters; 160 / 4 = 40 a level down


# ---- the definitions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 2])
def test_blend_np_in_crop_mode_is_forward_tiled(scale):
    """A numpy 'forward' that adds a tile-dependent constant (and upsamples by ``scale``): the stitched results agree bit for bit."""
    H, W, tile, overlap = 37, 53, 16, 4
    rng = np.random.default_rng(3)
    x = rng.random((1, 3, H, W), dtype=np.float32)
    counter = [0]

    def forward(t):
        out = []
        for k in range(t.shape[0]):
            counter[0] += 1
            out.append(np.repeat(np.repeat(t[k].numpy(), scale, axis=1), scale, axis=2) + np.float32(counter[0]))
        return torch.from_numpy(np.stack(out))

    want = forward_tiled(forward, torch.from_numpy(x), tile=tile, overlap=overlap, scale=scale, batch=5).numpy()[0]
    p = restore.plan(H, W, tile, overlap, scale=scale, blend="crop")
    counter[0] = 0
    tiles = forward(torch.from_numpy(restore.gather_np(x[0], p, 0, p.T, layout="chw"))).numpy()
    got = restore.blend_np(tiles, p, out="float32", layout="chw", clip=False)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert np.array_equal(restore.blend_np(tiles, p, out="float32", layout="hwc", clip=False), got.transpose(1, 2, 0))


def test_gather_np_converts_uint8_by_the_rounded_quotient():
    case = rc.CASES[0]
    im, p = rc.image(case), rc.plan_of(case)
    g = rc.gathered(case)
    assert g.shape == (p.T, 3, 16, 16) and g.dtype == np.float32
    y, x = p.boxes[7]
    assert np.array_equal(g[7], (im[y:y + 16, x:x + 16].transpose(2, 0, 1) / 255.0).astype(np.float32))
    assert (g != (im.astype(np.float32) * np.float32(1 / 255.0)).transpose(2, 0, 1)[:, :16, :16][None]).any()      # not the multiply
    assert np.array_equal(restore.gather_np(im, p, 3, 9), g[3:9])


def test_a_nan_tile_pollutes_only_its_support():
    case = rc.CASES[0]
    for blend in restore.BLENDS:
        p = rc.plan_of(case, 2, blend)
        tiles = rc.stack(case, 2).copy()
        bad = 9                                                                               # an inner tile: neighbours on every side
        tiles[bad] = np.nan
        got = restore.blend_np(tiles, p, out="float32", layout="chw")
        y, x = (v * 2 for v in p.boxes[bad])
        inside = np.zeros(got.shape[1:], dtype=bool)
        inside[y:y + p.tho, x:x + p.two] = True
        nan = np.isnan(got).all(axis=0)
        assert np.array_equal(np.isnan(got).any(axis=0), nan)
        assert not nan[~inside].any() and nan.any()
        if blend == "linear":
            assert nan[inside].all()                                                          # every pixel under the tile carries its weight
        clean = rc.blended(case, 2, blend, "float32", "chw")
        assert np.array_equal(got[:, ~nan], clean[:, ~nan])


def test_uint8_output_is_the_quantised_float_output():
    case = rc.CASES[0]
    for blend in restore.BLENDS:
        f = rc.blended(case, 1, blend, "float32", "hwc")
        assert f.min() == 0 and f.max() == 1
        assert np.array_equal(rc.blended(case, 1, blend, "uint8", "hwc"), np.rint(f.astype(np.float64) * 255).astype(np.uint8))


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    with pytest.raises(ValueError, match="twice the overlap"):
        restore.plan(100, 100, 16, 8)
    with pytest.raises(ValueError, match="under 4 tiles.*larger tile or a smaller overlap"):
        restore.plan(100, 100, 16, 6)
    restore.plan(100, 100, 16, 6, blend="crop")                                               # (crop needs one slot only)
    with pytest.raises(ValueError, match=r"stack of \d+ restored tiles.*smaller image band or a larger tile"):
        restore.plan(20000, 20000, 64, 24)
    with pytest.raises(ValueError, match="2\\^31 elements"):
        restore.plan(30000, 30000, 512, 32)
    with pytest.raises(ValueError, match="blend"):
        restore.plan(64, 64, 16, 4, blend="cosine")
    with pytest.raises(ValueError, match="at most 4"):
        restore.plan(64, 64, 16, 4, channels=5)
    p = restore.plan(37, 53, 16, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        restore.gather(torch.zeros(37, 53, 3, dtype=torch.uint8), p, 0, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        restore.blend(torch.zeros(p.T, 3, 16, 16), p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        restore.restore_tiles(lambda t: t, torch.zeros(37, 53, 3, dtype=torch.uint8), p)
    with pytest.raises(ValueError, match="5 channels"):
        restore.gather_np(np.zeros((37, 53, 5), dtype=np.uint8), p, 0, 1)
    with pytest.raises(ValueError, match="5 channels"):
        restore.gather(torch.zeros(37, 53, 5, dtype=torch.uint8), p, 0, 1)
    with pytest.raises(TypeError, match="uint8 or float32"):
        restore.gather_np(np.zeros((37, 53, 3), dtype=np.float64), p, 0, 1)
    with pytest.raises(ValueError, match="made for 37x53"):
        restore.gather_np(np.zeros((38, 53, 3), dtype=np.uint8), p, 0, 1)
    with pytest.raises(ValueError, match="24 tiles"):
        restore.gather_np(np.zeros((37, 53, 3), dtype=np.uint8), p, 3, 25)
    with pytest.raises(ValueError, match=r"\[24,C,16,16\]"):
        restore.blend_np(np.zeros((23, 3, 16, 16), dtype=np.float32), p)
    with pytest.raises(ValueError, match="out"):
        restore.blend_np(np.zeros((24, 3, 16, 16), dtype=np.float32), p, out="float16")
    assert p.resident_bytes(outputs=(3, 1)) > 37 * 53 * 3 + p.stack_elements(4) * 4
