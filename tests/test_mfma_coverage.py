"""tests/mfma_cases.py against the tile rule and the dispatch list of csrc/conv_mfma.hip, without a device.

1. Every row, under its knobs, reports its instantiation from virnet_conv_mfma_tile (the same pick_tile the launch runs), and its partner
   reports <KS, STRIDE, 1, 1> with four waves.
2. The rows together reach EXACTLY the instantiations the host can launch.  The set is written out below by hand from the VIRNET_CASE list
   and held to that list's text, so adding or removing a VIRNET_CASE without a row -- or a rule change that strands one -- fails here.
3. With the knobs unset pick_tile's thresholds sit where the code says: single slabs below 1024 four-row tiles, eight-row tiles from 2048
   eight-row tiles, eight waves from 512 (stride 2, two or three packed slabs -- four would ask for more LDS than a CU has).
4. The table holds what it was specified to hold (operand sets, depths, shapes).
5. The host refuses the descriptors it must refuse, and says which check refused them."""
import ctypes
import os
import re

import pytest

from mfma_cases import BY_ID, DEPTHS, OPS, P_OPS, REDZONE, ROWS, T_OPS, CROP
from virnet_amd import _native, ops

KNOBS = ("VIRNET_FORCE_MREP", "VIRNET_FORCE_NREP", "VIRNET_FORCE_NW")
N14, N13 = (1, 2, 3, 4, 5, 7), (1, 2, 3)
# conv_mfma.hip, the VIRNET_CASE list: (KS, STRIDE, MREP, NREP, NW)
DISPATCH = ({(ks, 1, 1, n, 4) for ks in (3, 1) for n in N14} | {(ks, 1, 2, n, 4) for ks in (3, 1) for n in N13}
            | {(3, 2, 1, n, 4) for n in N14} | {(3, 2, 1, n, 8) for n in (2, 3)})


def desc(kind="conv", stride=1, cin=96, cout=96, n=2, h=5, w=33, **fields):
    """The descriptor ops.conv_mfma / conv_mfma_nchw builds, with dummy non-NULL pointers (pick_tile and the checks only test them for NULL)."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ks = 3 if kind in ("conv", "planar") else 1
    plan = ops.get_plan(ks, stride, cin, 4 * cout if kind == "convt" else cout)
    assert plan.cin_pad == cin
    epi = {"conv": _native.EPI_NHWC, "dgemm": _native.EPI_NHWC, "convt": _native.EPI_CONVT, "planar": _native.EPI_NCHW}[kind]
    d = _native.ConvDesc(x=p, wpack=p, bias=p, y_raw=p, n=n, h=h, w=w, cin_pad=cin, cout=cout, ks=ks, stride=stride, epi=epi, n_pad=plan.n_pad,
                         nrep=plan.nrep, slope=0.2, mask_slope=0.2, res_sf=1, crop_h=h, crop_w=w)
    for k, v in fields.items():
        setattr(d, k, p if v == "ptr" else v)
    d._keep = buf
    return d


def desc_for(row):
    d = desc(row.kind, row.stride, row.cin, row.cout, row.n, row.h, row.w)
    if row.kind == "planar":
        d.crop_h, d.crop_w = CROP(row)
    return d


def tile(d, monkeypatch, env=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    out = (ctypes.c_int * 5)()
    _native.check(_native.load().virnet_conv_mfma_tile(ctypes.byref(d), ctypes.byref(out)), "conv_mfma_tile")
    var = (ctypes.c_int * 4)()
    _native.check(_native.load().virnet_conv_mfma_variant(ctypes.byref(d), ctypes.byref(var)), "conv_mfma_variant")
    assert tuple(var) == tuple(out)[:4]                    # the launch timer's key (bench.py) is the same rule
    return tuple(out)


def test_rows_report_the_instantiation_they_record(monkeypatch):
    bad = []
    for row in ROWS:
        d = desc_for(row)
        got, single = tile(d, monkeypatch, row.env), tile(d, monkeypatch, row.single)
        if got != row.tile or single != (row.ks, row.stride, 1, 1, 4):
            bad.append((row.id, got, single))
        assert row.tile[:2] == (row.ks, row.stride) and (row.tile[2] * row.tile[4] + 1) * row.stride == (row.h if row.kind != "planar" else row.h - 2), row.id
        # small shapes: without the knobs every row is the single-slab, four-row, four-wave launch -- the gap this table closes
        assert tile(d, monkeypatch) == (row.ks, row.stride, 1, 1, 4), row.id
    assert not bad, f"{len(bad)} of {len(ROWS)} rows differ, first: {bad[:3]}"


def test_table_reaches_exactly_the_dispatch_list():
    got = {r.tile for r in ROWS}
    assert not DISPATCH - got, sorted(DISPATCH - got)
    assert not got - DISPATCH, sorted(got - DISPATCH)
    assert len(DISPATCH) == 26
    # ... and the hand-written set is the VIRNET_CASE list of the source, in both directions
    with open(os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc", "conv_mfma.hip")) as f:
        src = f.read()
    body = src[src.index("#define VIRNET_CASE("):src.index("#undef VIRNET_CASE")]
    cases = [tuple(int(v) for v in m) for m in re.findall(r"VIRNET_CASE\((\d), (\d), (\d), (\d), (\d)\);", body)]
    assert len(cases) == len(set(cases)) == body.count("VIRNET_CASE(") - 1, "a VIRNET_CASE this test cannot read"
    assert set(cases) == DISPATCH, (sorted(set(cases) - DISPATCH), sorted(DISPATCH - set(cases)))
    assert "launch<" not in src[src.index("#undef VIRNET_CASE"):], "a launch outside the VIRNET_CASE list"


@pytest.mark.parametrize("kind,stride,cout,n,h,w,want", [
    # 96 channels = one block of three slabs.  4 x 32 outputs per image: n four-row tiles, n eight-row tiles
    ("conv", 1, 96, 1023, 4, 32, (3, 1, 1, 1, 4)), ("conv", 1, 96, 1024, 4, 32, (3, 1, 1, 3, 4)),
    # 8 x 32 outputs per image: 2n four-row tiles, n eight-row tiles
    ("conv", 1, 96, 2047, 8, 32, (3, 1, 1, 3, 4)), ("conv", 1, 96, 2048, 8, 32, (3, 1, 2, 3, 4)),
    # 192 channels = two blocks: the thresholds count workgroups, tiles x blocks
    ("conv", 1, 192, 511, 4, 32, (3, 1, 1, 1, 4)), ("conv", 1, 192, 512, 4, 32, (3, 1, 1, 3, 4)), ("conv", 1, 192, 1024, 8, 32, (3, 1, 2, 3, 4)),
    # four packed slabs and more never take eight-row tiles
    ("conv", 1, 128, 4096, 8, 32, (3, 1, 1, 4, 4)), ("dgemm", 1, 160, 4096, 8, 32, (1, 1, 1, 5, 4)),
    # the transposed conv to 96 channels: 12 slabs = four blocks of three
    ("convt", 1, 96, 511, 8, 32, (1, 1, 1, 3, 4)), ("convt", 1, 96, 512, 8, 32, (1, 1, 2, 3, 4)),
    # stride 2 (16 x 64 inputs = 8 x 32 outputs): eight waves from 512 eight-row tiles, where the packed grouping is kept (1024 four-row tiles)
    ("conv", 2, 96, 511, 16, 64, (3, 2, 1, 1, 4)), ("conv", 2, 96, 512, 16, 64, (3, 2, 1, 3, 8)), ("conv", 2, 64, 512, 16, 64, (3, 2, 1, 2, 8)),
    ("conv", 2, 96, 1023, 8, 64, (3, 2, 1, 1, 4)), ("conv", 2, 96, 1024, 8, 64, (3, 2, 1, 3, 8)),
    # ... with 2 or 3 packed slabs only: <3,2,1,4,8> would ask for 166 016 B of LDS
    ("conv", 2, 128, 512, 16, 64, (3, 2, 1, 4, 4)), ("conv", 2, 128, 8, 256, 256, (3, 2, 1, 4, 4)), ("conv", 2, 160, 512, 16, 64, (3, 2, 1, 5, 4)),
    ("conv", 2, 32, 512, 16, 64, (3, 2, 1, 1, 4)), ("conv", 2, 288, 512, 16, 64, (3, 2, 1, 3, 8))])
def test_thresholds_with_the_knobs_unset(monkeypatch, kind, stride, cout, n, h, w, want):
    assert tile(desc(kind, stride, 32, cout, n, h, w), monkeypatch) == want


def test_eight_wave_edge_alone_and_what_the_knobs_may_pin(monkeypatch):
    d511, d512 = desc("conv", 2, 32, 96, 511, 16, 64), desc("conv", 2, 32, 96, 512, 16, 64)
    assert tile(d511, monkeypatch, {"VIRNET_FORCE_NREP": "3"}) == (3, 2, 1, 3, 4)          # the packed grouping pinned: 511 / 512 by itself
    assert tile(d512, monkeypatch, {"VIRNET_FORCE_NREP": "3"}) == (3, 2, 1, 3, 8)
    assert tile(d512, monkeypatch, {"VIRNET_FORCE_NW": "4"}) == (3, 2, 1, 3, 4)
    assert tile(d512, monkeypatch, {"VIRNET_FORCE_NREP": "1"}) == (3, 2, 1, 1, 4)          # single slabs run four waves
    small = dict(n=2, h=18, w=66)
    # VIRNET_FORCE_NW=8 is honoured exactly where an 8-wave instantiation exists
    assert tile(desc("conv", 2, 32, 96, **small), monkeypatch, {"VIRNET_FORCE_NW": "8", "VIRNET_FORCE_NREP": "3"}) == (3, 2, 1, 3, 8)
    assert tile(desc("conv", 2, 32, 96, **small), monkeypatch, {"VIRNET_FORCE_NW": "8"}) == (3, 2, 1, 1, 4)
    assert tile(desc("conv", 2, 32, 128, **small), monkeypatch, {"VIRNET_FORCE_NW": "8", "VIRNET_FORCE_NREP": "4"}) == (3, 2, 1, 4, 4)
    assert tile(desc("conv", 2, 32, 32, **small), monkeypatch, {"VIRNET_FORCE_NW": "8"}) == (3, 2, 1, 1, 4)
    assert tile(desc("conv", 1, 32, 96, n=2, h=9, w=33), monkeypatch, {"VIRNET_FORCE_NW": "8", "VIRNET_FORCE_NREP": "3"}) == (3, 1, 1, 3, 4)
    # eight-row tiles: stride 1, at most three packed slabs; a slab count other than 1 or the packed one is ignored
    assert tile(desc("conv", 1, 32, 128, n=2, h=9, w=33), monkeypatch, {"VIRNET_FORCE_MREP": "2", "VIRNET_FORCE_NREP": "4"}) == (3, 1, 1, 4, 4)
    assert tile(desc("conv", 2, 32, 96, **small), monkeypatch, {"VIRNET_FORCE_MREP": "2", "VIRNET_FORCE_NREP": "3"}) == (3, 2, 1, 3, 4)
    assert tile(desc("conv", 1, 32, 96, n=2, h=9, w=33), monkeypatch, {"VIRNET_FORCE_NREP": "2"}) == (3, 1, 1, 1, 4)
    # read per call: the same process, the same descriptor, another answer
    d = desc("conv", 1, 32, 96, n=2, h=9, w=33)
    assert [tile(d, monkeypatch, {"VIRNET_FORCE_MREP": m, "VIRNET_FORCE_NREP": n})[2:4] for m, n in (("2", "3"), ("1", "1"), ("2", "1"))] == [(2, 3), (1, 1), (2, 1)]


def test_table_holds_what_it_must():
    fam = lambda r: (r.ks, r.stride)
    nhwc = [r for r in ROWS if r.kind in ("conv", "dgemm")]
    for f in ((3, 1), (3, 2), (1, 1)):
        rows = [r for r in ROWS if fam(r) == f]
        assert {r.ops for r in rows if r.kind in ("conv", "dgemm")} == set(OPS), f          # every operand set once per family
        assert any(r.n == 3 for r in rows), f                                               # 12 tiles: two per XCD, four idle slots
        assert {r.cin for r in rows} >= set(DEPTHS), f                                      # 1, 2, 3 chunks
        # ... all of them on the three-slab rows, and on the eight-row rows where the family has them
        assert {r.ops for r in nhwc if fam(r) == f and r.tile[3] == 3 and r.cout == 96} == set(OPS), f
        if f != (3, 2):
            assert {r.ops for r in nhwc if fam(r) == f and r.tile[2] == 2} == set(OPS), f
    assert {r.ops for r in nhwc if r.tile == (3, 2, 1, 3, 8)} == set(OPS)
    convt = [r for r in ROWS if r.kind == "convt"]
    assert {r.ops for r in convt} == set(T_OPS) == {r.ops for r in convt if r.tile[2] == 2}
    assert {r.cout for r in convt} == {96, 32, 64, 160} and {r.tile[3] for r in convt} == {1, 3, 4}
    assert {(r.cout, r.tile[3]) for r in ROWS if r.kind == "dgemm"} == {(64, 2), (96, 3), (160, 5), (224, 7)}
    assert any(r.kind == "dgemm" and r.cin == 16 and r.tile[2:4] == (1, 2) for r in ROWS)    # ks = 1, one stage
    assert {(r.cin, r.cout) for r in ROWS if r.cin > 48} == {(288, 288), (224, 224)}
    assert {(r.cout, r.tile[3]) for r in ROWS if r.kind == "conv" and r.tile[3] > 1} == {
        (64, 2), (96, 3), (192, 3), (288, 3), (128, 4), (160, 5), (224, 7)}
    # shapes: one partial tile on each axis, the last with a single column
    for r in ROWS:
        th = r.tile[2] * r.tile[4]
        oh, ow = r.h // r.stride, r.w // r.stride
        assert r.n in (2, 3) and r.h % r.stride == 0 and r.w % r.stride == 0
        assert (oh, ow) == ((th + 3, 36) if r.kind == "planar" else (th + 1, 33)), r.id
    planar = [r for r in ROWS if r.kind == "planar"]
    for m in (1, 2):
        rows = [r for r in planar if r.tile == (3, 1, m, 1, 4)]
        assert {r.cout for r in rows} == {1, 3, 5, 17, 32} and {r.ops for r in rows} == set(P_OPS)
        assert all(CROP(r)[0] < r.h and CROP(r)[1] < r.w and CROP(r)[0] % 2 == 0 and CROP(r)[1] % 2 == 0 for r in rows)
    assert len({r.seed for r in ROWS}) == len(ROWS)                                          # another weight per row
    # the red-zone list: per (KS, STRIDE, MREP, NW) the largest and the smallest NREP of the table, and the planar rows with 5 and 32 channels
    assert len(set(REDZONE)) == len(REDZONE) and all(rid in BY_ID for rid in REDZONE)
    red = [BY_ID[rid] for rid in REDZONE]
    for key in {(r.ks, r.stride, r.tile[2], r.tile[4]) for r in ROWS}:
        nreps = {r.tile[3] for r in ROWS if (r.ks, r.stride, r.tile[2], r.tile[4]) == key and r.kind != "planar"}
        got = {r.tile[3] for r in red if (r.ks, r.stride, r.tile[2], r.tile[4]) == key and r.kind != "planar"}
        assert {min(nreps), max(nreps)} <= got, (key, nreps, got)
    assert {(r.tile[2], r.cout) for r in red if r.kind == "planar"} == {(1, 5), (1, 32), (2, 5), (2, 32)}


REJECT = [
    # (what, descriptor arguments, the words of the check that must refuse it)
    ("planar store with a pointwise packing", dict(kind="planar", cin=96, cout=3, ks=1), "planar store needs ks=3"),
    ("mul without add", dict(mul="ptr"), "mul and add must be given together"),
    ("add without mul", dict(add="ptr"), "mul and add must be given together"),
    ("odd stride-2 height", dict(stride=2, h=9, w=66), "must be even"),
    ("odd stride-2 width", dict(stride=2, h=10, w=65), "must be even"),
    ("NHWC store of the padded rows", dict(cout=90, n_pad=96), "to be a multiple of 32"),
    ("transposed store with a 3x3 packing", dict(kind="convt", ks=3), "transposed-conv store needs ks=1"),
    ("planar store of 33 channels", dict(kind="planar", cout=33), "planar store handles 1..32 channels"),
    ("crop beyond the output's rows", dict(kind="planar", cout=3, crop_h=6), "outside output"),
    ("crop beyond the output's columns", dict(kind="planar", cout=3, crop_w=34), "outside output"),
    ("in_mul without in_act", dict(in_mul="ptr", in_add="ptr"), "in_mul/in_add without in_act"),
    ("in_mul without in_add", dict(in_mul="ptr", in_act=1), "in_mul and in_add must be given together"),
]


@pytest.mark.parametrize("what,args,words", REJECT, ids=[r[0].replace(" ", "_") for r in REJECT])
def test_host_refuses_and_names_the_check(what, args, words):
    """Through virnet_conv_mfma_check -- the checks of virnet_conv_mfma and nothing after them -- so that a check that stopped refusing
    fails this test on a machine with a device too, instead of launching a kernel on the dummy pointers."""
    d = desc(**args)
    lib = _native.load()
    assert lib.virnet_conv_mfma_check(ctypes.byref(d)) != 0, what
    msg = lib.virnet_last_error().decode()
    assert msg.startswith("virnet_conv_mfma:") and words in msg, (what, msg)


def test_check_accepts_every_row_and_the_tile_query_refuses_what_it_would_divide_by():
    lib = _native.load()
    for row in ROWS:
        assert lib.virnet_conv_mfma_check(ctypes.byref(desc_for(row))) == 0, (row.id, lib.virnet_last_error())
    assert lib.virnet_conv_mfma_check(None) != 0
    out = (ctypes.c_int * 5)()
    for field in ("nrep", "stride"):
        d = desc()
        setattr(d, field, 0)
        assert lib.virnet_conv_mfma_tile(ctypes.byref(d), ctypes.byref(out)) != 0
        assert "virnet_conv_mfma_tile: nrep=" in lib.virnet_last_error().decode()


@pytest.mark.parametrize("family", ["PLAN_F16", "PLAN_BF16", "PLAN_WX4", "PLAN_WX4X1"])
@pytest.mark.parametrize("field", ["mul", "add"])
def test_split_fp16_hosts_pair_mul_and_add(family, field):
    """conv_f16_common.h's check_conv_desc, through the plan query: the checks of the launch entries without their launch."""
    with pytest.raises(RuntimeError, match="mul and add must be given together"):
        ops.conv_plan_query(getattr(_native, family), desc(**{field: "ptr"}))
    assert ops.conv_plan_query(getattr(_native, family), desc(mul="ptr", add="ptr", y_act="ptr"))


@pytest.mark.parametrize("field", ["mul", "add"])
def test_winograd_host_pairs_mul_and_add(field):
    """virnet_conv_wino has no entry that stops after its checks, so this goes through the launch entry: the descriptor is one that the
    new check refuses BEFORE anything touches the runtime -- should the check ever be removed, this case has to go with it, not be
    left to launch on the dummy pointers."""
    d = desc(**{field: "ptr"})
    lib = _native.load()
    assert lib.virnet_conv_wino(ctypes.byref(d), None) != 0
    assert "virnet_conv_wino: mul and add must be given together" in lib.virnet_last_error().decode()
