"""tests/variant_cases.py against the launch rules and the dispatch code, without a device.

1. Every row, under its knobs, plans exactly the launches it records (virnet_conv_plan_query at 256 and at 64 CUs: a pinned plan does not
   depend on the CU count), and its single-slab partner plans single slabs.
2. The rows together reach EVERY instantiation the dispatch code can launch -- the set is written out below from
   launch_wx4_planned (conv_f16_wx4.hip), launch_wx4h (conv_f16_wx4h.hip), launch_f16_planned (conv_f16.hip), launch_f16_s2
   (conv_f16_s2.hip) and launch_f16_convt (conv_f16_pw.hip) -- so a later plan rule cannot take an instantiation out of the kernel-level
   tests without this file noticing.  T emission, the entry / planar forms and the persistent form have tests of their own.
3. The table is exactly the rows the list below asks for: deleting one fails here."""
import ctypes

import pytest

from test_launch_plan import KNOBS, LAUNCH
from variant_cases import EPI_CLASS, RANGE_GUARD, ROWS, reached
from virnet_amd import _native, ops

FAMILY = {"wx4": _native.PLAN_WX4, "f16": _native.PLAN_F16, "bf16": _native.PLAN_BF16, "s2": _native.PLAN_F16, "convt": _native.PLAN_F16}
PY_KNOBS = ("VIRNET_CONV_FORM", "VIRNET_WX4_MIN_TILES", "VIRNET_WX4_MIN_COUT", "VIRNET_WX4_MIN_FILL")      # read by ops.py, not by the plan

EPIS, PRES = range(5), range(3)
DISPATCH = (
    # launch_wx4_planned: VIRNET_WX4_CASE(3) (2) (1), each VIRNET_WX4_EPI 0..4 x pre 2 / 1 / 0
    {("wx4", 16, 1, nrep, 0, e, p) for nrep in (1, 2, 3) for e in EPIS for p in PRES}
    # launch_wx4h: VIRNET_WX4H_CASE(3) (2) (1) (5), the same epilogues
    | {("wx4h", 8, 1, nrep, 0, e, p) for nrep in (1, 2, 3, 5) for e in EPIS for p in PRES}
    # launch_f16_planned: VIRNET_F16_CASE(2|1, 3|2|1), epi 0..4, split-fp16 and bf16 operands (the pre-activation is a run-time branch)
    | {(fam, 4 * m, 1, nrep, m, e, None) for fam in ("f16", "bf16") for m in (1, 2) for nrep in (1, 2, 3) for e in EPIS}
    # launch_f16_s2: <1,1> <1,5> <1,7> <1,4> <2,3> <1,3> <1,2>
    | {("s2", 4, ng, nrep, 0, None, None) for ng, nrep in ((1, 1), (1, 5), (1, 7), (1, 4), (2, 3), (1, 3), (1, 2))}
    # launch_f16_convt: <2,3> <1,3> <1,2>, KS 2 and 3.  (<1,1> is in the code and in no plan: variant_cases._convt_rows says why.)
    | {("convt", 0, ng, nrep, ks, None, None) for ng, nrep in ((2, 3), (1, 3), (1, 2)) for ks in (2, 3)})


def desc_for(row):
    """The descriptor ops.conv_mfma builds for a row, with dummy non-NULL pointers (the plan only tests them for NULL)."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    d = _native.ConvDesc(x=p, wpack=p, bias=p, n=row.n, h=row.h, w=row.w, cin_pad=row.cin, cout=row.cout, ks=3, stride=1, epi=_native.EPI_NHWC,
                         n_pad=row.cout, nrep=1, slope=0.2, mask_slope=0.2)
    if row.family == "s2":
        d.stride, d.y_raw = 2, p
    elif row.family == "convt":
        d.ks, d.epi, d.n_pad = 1, _native.EPI_CONVT, 4 * row.cout
        if row.ops[0]:
            d.res, d.y_raw = p, p
        else:
            d.y_act = p
    else:
        epi, pre = row.ops
        if epi in ("res", "mask_res", "dual", "sft"):
            d.res = p
        if epi in ("mask", "mask_res"):
            d.mask = p
        if epi == "sft":
            d.mul = d.add = p
        if epi != "act":
            d.y_raw = p
        if epi in ("act", "dual", "sft"):
            d.y_act = p
        if pre >= 1:
            d.in_act, d.in_slope = 1, 0.2
        if pre == 2:
            d.in_mul = d.in_add = p
    d._keep = buf
    return d


def plan(row, env, n_cu, monkeypatch):
    for k in KNOBS + PY_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return [tuple(l[k] for k in LAUNCH) for l in ops.conv_plan_query(FAMILY[row.family], desc_for(row), n_cu=n_cu)]


@pytest.mark.parametrize("n_cu", [256, 64])
def test_rows_plan_the_launches_they_record(monkeypatch, n_cu):
    bad = []
    for row in ROWS:
        got, single = plan(row, row.env, n_cu, monkeypatch), plan(row, row.single, n_cu, monkeypatch)
        if got != row.launches or single != row.single_launches:
            bad.append((row.id, row.launches, got, row.single_launches, single))
        # the descriptor spells the operand set the row names
        if row.family in ("wx4", "f16", "bf16"):
            d = desc_for(row)
            epi = 4 if (d.mul or (d.y_raw and d.y_act)) else (1 if d.res else 0) | (2 if d.mask else 0)
            assert (epi, 2 if d.in_mul else d.in_act) == (EPI_CLASS[row.ops[0]], row.ops[1]), row.id
    assert not bad, f"{len(bad)} of {len(ROWS)} rows differ, first: {bad[:3]}"


def test_pinned_rows_run_more_than_one_slab_and_partners_run_the_smallest_grouping():
    for row in ROWS:
        assert all(ng * nrep >= 2 for _, _, ng, nrep, *_ in row.launches), row.id
        smallest = 2 if row.family == "convt" else 1                      # (the transposed host has no single-slab plan: see variant_cases)
        assert all(ng == 1 and nrep == smallest for _, _, ng, nrep, *_ in row.single_launches), row.id


def test_table_reaches_every_dispatched_instantiation():
    """The partner runs count: test_conv_variants_gpu compares each with its row bit for bit, after the row met the fp64 reference."""
    got = set()
    for row in ROWS:
        got |= reached(row) | reached(row, row.single_launches)
    assert not DISPATCH - got, sorted(DISPATCH - got, key=str)
    assert not got - DISPATCH, sorted(got - DISPATCH, key=str)                # an instantiation the list above does not know: extend it
    # ... and the multi-slab ones are reached by pinned rows alone
    multi = {t for t in DISPATCH if t[2] * t[3] >= 2}
    pinned = set().union(*(reached(row) for row in ROWS))
    assert not multi - pinned, sorted(multi - pinned, key=str)


def required():
    """What the table must hold, spelled independently of its generators: (family, tile rows | MREP | None, cin, cout, knob that pins the
    grouping, n, h, w, epilogue class | bridge | None, pre | None)."""
    req = set()
    for r in (16, 8):
        shape = (2, r + 1, 33)
        for c in (96, 64):
            req |= {("wx4", r, c, c, "NREP=3", *shape, e, p) for e in EPIS for p in PRES}
        req |= {("wx4", r, 160, 160, "NREP=3", *shape, 0, 0), ("wx4", r, 224, 224, "NREP=3", *shape, 1, 1), ("wx4", r, 288, 288, "NREP=3", *shape, 2, 2),
                ("wx4", r, 48, 96, "NREP=3", *shape, 3, 0), ("wx4", r, 192, 192, "NREP=2", *shape, 4, 1)}
    req |= {("wx4", 8, 160, 160, "", 2, 9, 33, e, p) for e in EPIS for p in PRES}
    for m in (1, 2):
        shape = (2, 4 * m + 1, 33)
        for c in (96, 64):
            req |= {("f16", m, c, c, "SPLIT=0", *shape, e, p) for e in EPIS for p in PRES}
            req |= {("bf16", m, c, c, "SPLIT=0", *shape, e, e % 2) for e in EPIS}
        req |= {("f16", m, cin, cout, "SPLIT=0", *shape, (i + m) % 5, (i + m) % 3)
                for i, (cin, cout) in enumerate([(128, 128), (160, 160), (224, 224), (288, 288), (48, 96)])}
        req.add(("bf16", m, 160, 160, "SPLIT=0", *shape, m % 5, m % 2))
    req |= {("s2", None, cin, cout, "TILES=0", 2, 10, 66, None, None) for cin, cout in ((96, 128), (96, 160), (160, 224), (96, 192), (64, 64))}
    req.add(("s2", None, 48, 288, "TILES=0", 6, 122, 66, None, None))
    for cin, cout, pin in ((96, 192, ""), (96, 192, "KS=3"), (192, 160, "KS=3"), (288, 64, "KS=3"), (96, 32, "KS=3"), (48, 32, ""), (80, 32, ""), (80, 32, "KS=3"),
                           (96, 64, "KS=3 SLABS=3"), (96, 64, "SLABS=3")):
        req |= {("convt", None, cin, cout, pin, 2, 5, 33, bridge, None) for bridge in (True, False)}
    return req


def key_of(row):
    e = row.env
    if row.family == "wx4":
        return ("wx4", int(e["VIRNET_WX4_ROWS"]), row.cin, row.cout, "NREP=" + e["VIRNET_WX4_NREP"] if "VIRNET_WX4_NREP" in e else "",
                row.n, row.h, row.w, EPI_CLASS[row.ops[0]], row.ops[1])
    if row.family in ("f16", "bf16"):
        return (row.family, int(e["VIRNET_F16_MREP"]), row.cin, row.cout, "SPLIT=" + e["VIRNET_F16_SPLIT_WGS"], row.n, row.h, row.w,
                EPI_CLASS[row.ops[0]], row.ops[1])
    if row.family == "s2":
        return ("s2", None, row.cin, row.cout, "TILES=" + e["VIRNET_S2_SPLIT_TILES"], row.n, row.h, row.w, None, None)
    pin = " ".join(f"{k}={e['VIRNET_CONVT_' + k]}" for k in ("KS", "SLABS") if "VIRNET_CONVT_" + k in e)
    return ("convt", None, row.cin, row.cout, pin, row.n, row.h, row.w, row.ops[0], None)


def test_table_is_exactly_the_required_rows():
    keys = [key_of(r) for r in ROWS]
    assert len(set(keys)) == len(keys) == len({r.id for r in ROWS})
    req = required()
    assert not req - set(keys), sorted(req - set(keys), key=str)[:5]
    assert not set(keys) - req, sorted(set(keys) - req, key=str)[:5]
    # the row the issue singles out: 8-row tiles, three slabs AND the SFT table (the one-workgroup-per-CU LDS size of conv_wx4h)
    assert ("wx4", 8, 96, 96, "NREP=3", 2, 9, 33, 4, 2) in req
    ids = {r.id for r in ROWS}
    assert all(rid in ids for rid, _, _ in RANGE_GUARD)
