"""tests/t_emit_cases.py against the launch rules, the form rule and the emitting dispatch code, without a device.

1. Every row, under its knobs, plans exactly the launches it records (virnet_conv_plan_query with the row's emit_rows at 256 and at 64
   CUs), and the VIRNET_WX4_NREP=1 partner of a Winograd row plans single slabs.
2. Rows plus partners reach EVERY emitting instantiation the dispatch code can launch and nothing else -- DISPATCH_TE is written out below
   from VIRNET_WX4_TE (launch_wx4_planned, conv_f16_wx4.hip), VIRNET_WX4H_TE (launch_wx4h_emit, conv_f16_wx4h.hip) and VIRNET_F16_TE
   (launch_f16_planned, conv_f16.hip) -- and every multi-slab one is reached by a pinned row alone.
3. ops.conv_form_rule, on each row's plain values under the row's environment, sends the row to the family and the emitting tile height it
   records: the 8-row emitting Winograd kernels really are what ops.conv_mfma reaches for these shapes.
4. The table is exactly the rows the list below asks for: deleting one fails here."""
import pytest

from t_emit_cases import ROWS, emit_mode, plain_env, reached
from test_launch_plan import KNOBS, LAUNCH
from test_variant_coverage import FAMILY, PY_KNOBS, desc_for
from variant_cases import EPI_CLASS
from virnet_amd import ops

ALL_KNOBS = KNOBS + PY_KNOBS + ("VIRNET_WX4_EMIT_ROWS", "VIRNET_T_EMIT", "VIRNET_WINOGRAD", "VIRNET_WX4_MIN_SLAB_WGS")

EPIS = range(4)
DISPATCH_TE = (
    # launch_wx4_planned: VIRNET_WX4_TEN(3) (2) (1), each VIRNET_WX4_TE(N, 0..3) with PRE 1 / 0 -> launch_wx4<N, E, PRE, 1>
    {("wx4", 16, nrep, e, pre) for nrep in (1, 2, 3) for e in EPIS for pre in (0, 1)}
    # launch_wx4h_emit: VIRNET_WX4H_TEN(3) (2) (1), the same -> launch_wx4h_t<N, E, PRE, 1>
    | {("wx4h", 8, nrep, e, pre) for nrep in (1, 2, 3) for e in EPIS for pre in (0, 1)}
    # launch_f16_planned: VIRNET_F16_TEN(3) (2) (1), each VIRNET_F16_TE(N, 0..3) with bf16 operands 0 / 1 -> launch<2, N, E, BF, 1>
    | {("f16", 8, nrep, e, bf) for nrep in (1, 2, 3) for e in EPIS for bf in (0, 1)})


def clear(monkeypatch, env):
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def plan(row, env, n_cu, monkeypatch, emit=True):
    clear(monkeypatch, env)
    return [tuple(l[k] for k in LAUNCH) for l in ops.conv_plan_query(FAMILY[row.family], desc_for(row), emit_rows=row.emit_rows if emit else 0, n_cu=n_cu)]


def test_dispatch_set_has_72_instantiations():
    assert len(DISPATCH_TE) == 72


@pytest.mark.parametrize("n_cu", [256, 64])
def test_rows_plan_the_launches_they_record(monkeypatch, n_cu):
    bad = []
    for row in ROWS:
        got = plan(row, row.env, n_cu, monkeypatch)
        single = plan(row, row.single, n_cu, monkeypatch) if row.family == "wx4" else None
        # the non-emitting call the device test compares with, under plain_env: the same launches
        plain = plan(row, plain_env(row), n_cu, monkeypatch, emit=False)
        if got != row.launches or single != row.single_launches or plain != row.launches:
            bad.append((row.id, row.launches, got, row.single_launches, single, plain))
        assert (row.single is None) == (row.family != "wx4"), row.id
        # the descriptor spells the operand set the row names: one stored tensor, no output SFT
        d = desc_for(row)
        assert not d.mul and bool(d.y_raw) != bool(d.y_act), row.id
        assert ((1 if d.res else 0) | (2 if d.mask else 0), 2 if d.in_mul else d.in_act) == (EPI_CLASS[row.ops[0]], row.ops[1]), row.id
        assert bool(d.y_act) == (row.ops[0] == "act") == (emit_mode(row)["colsum"] is None), row.id
    assert not bad, f"{len(bad)} of {len(ROWS)} rows differ, first: {bad[:3]}"


def test_partners_run_single_slabs_and_emit_rows_match_the_family():
    for row in ROWS:
        if row.family == "wx4":
            assert row.emit_rows in (16, 8) and all(l[1] == row.emit_rows for l in row.launches + row.single_launches), row.id
            assert all(ng == 1 and nrep == 1 for _, _, ng, nrep, *_ in row.single_launches), row.id
            assert sum(l[6] for l in row.single_launches) == row.cout // 32
        else:
            assert row.emit_rows == 8 and all(l[1] == 8 and l[4] == 2 for l in row.launches), row.id
        # the launches cover the slabs once, in order
        base = 0
        for _, _, ng, nrep, _, slab_base, groups, _ in row.launches:
            assert slab_base == base, row.id
            base += ng * nrep * groups
        assert base == row.cout // 32, row.id


def test_table_reaches_every_emitting_instantiation():
    """The partner runs count: test_t_emit_variants_gpu compares each with its row bit for bit, after the row met the references."""
    got = set()
    for row in ROWS:
        got |= reached(row)
        if row.family == "wx4":
            got |= reached(row, row.single_launches)
    assert not DISPATCH_TE - got, sorted(DISPATCH_TE - got, key=str)
    assert not got - DISPATCH_TE, sorted(got - DISPATCH_TE, key=str)          # an instantiation the list above does not know: extend it
    multi = {t for t in DISPATCH_TE if t[2] >= 2}
    pinned = set().union(*(reached(row) for row in ROWS))
    assert not multi - pinned, sorted(multi - pinned, key=str)
    # the single-slab emitting launch away from slab 0, and the second / third launch of a mixed grouping
    assert any(l[3] == 1 and l[5] == 4 for row in ROWS if row.family == "wx4" for l in row.launches)
    for r in (16, 8):
        bases = {l[5] for row in ROWS if row.family == "wx4" and row.emit_rows == r for l in row.launches}
        assert bases == {0, 3, 4}, (r, bases)                                 # (224 channels: slabs 3-4 and 5-6 are the two groups of the launch at 3)


def test_form_rule_sends_every_row_to_its_family_and_tile_height(monkeypatch):
    for row in ROWS:
        clear(monkeypatch, row.env)
        name, pre = row.ops
        got = ops.conv_form_rule(False, True, row.family == "bf16", row.family == "wx4", False, 1, True, row.n, row.h, row.w, row.cin, row.cout,
                                 name in ("res", "mask_res"), name in ("mask", "mask_res"), False, pre == 2, name != "act", name == "act", True)
        want = ("wx4", row.emit_rows) if row.family == "wx4" else ("f16x3" if row.family == "f16" else "bf16", 0)
        assert got == want, (row.id, got, want)
        if row.family == "wx4":
            # at the smallest launch the rule keeps on the Winograd form: one image fewer goes to the direct kernel
            wgs = lambda n: n * ((row.h + 15) // 16) * ((row.w + 31) // 32) * ((row.cout + 95) // 96)
            assert wgs(row.n) >= ops.WX4_EMIT_MIN_WGS > wgs(row.n - 1), row.id
            assert "VIRNET_WX4_MIN_WGS" not in row.env and "VIRNET_DETERMINISTIC" not in row.env


def required():
    """What the table must hold, spelled independently of its generators: (family, emit tile rows, cin, cout, knob that pins the grouping,
    n, h, w, epilogue class, pre)."""
    req = set()
    for r in (16, 8):
        for c in (96, 64):
            req |= {("wx4", r, c, c, "NREP=3", 32, 17, 33, e, p) for e in EPIS for p in (0, 1)}
        req |= {("wx4", r, 160, 160, "NREP=3", 16, 17, 33, 0, 0), ("wx4", r, 224, 224, "NREP=3", 11, 17, 33, 1, 1), ("wx4", r, 288, 288, "NREP=3", 11, 17, 33, 2, 0),
                ("wx4", r, 48, 96, "NREP=3", 32, 17, 33, 3, 1), ("wx4", r, 192, 96, "NREP=3", 32, 17, 33, 0, 0),
                ("wx4", r, 192, 192, "NREP=2", 16, 17, 33, 2, 1), ("wx4", r, 160, 160, "NREP=2", 16, 17, 33, 1, 0),
                ("wx4", r, 96, 96, "NREP=3", 64, 17, 31, 1, 0)}
    shape = (2, 9, 33)
    req |= {("f16", 8, 96, 96, "", *shape, e, p) for e in EPIS for p in (0, 1, 2)}
    for c in (64, 32):
        req |= {("f16", 8, c, c, "", *shape, e, e % 3) for e in EPIS}
    req |= {("f16", 8, 128, 128, "", *shape, 0, 0), ("f16", 8, 160, 160, "", *shape, 1, 1), ("f16", 8, 224, 224, "", *shape, 2, 2),
            ("f16", 8, 288, 288, "", *shape, 3, 0), ("f16", 8, 48, 96, "", *shape, 0, 1), ("f16", 8, 192, 96, "", *shape, 1, 2),
            ("f16", 8, 96, 96, "", 2, 9, 31, 1, 0)}
    for c in (96, 64, 32):
        req |= {("bf16", 8, c, c, "", *shape, e, e % 2) for e in EPIS}
    req.add(("bf16", 8, 160, 160, "", *shape, 1, 1))
    return req


def key_of(row):
    e = row.env
    pin = "NREP=" + e["VIRNET_WX4_NREP"] if row.family == "wx4" else ""
    return (row.family, row.emit_rows, row.cin, row.cout, pin, row.n, row.h, row.w, EPI_CLASS[row.ops[0]], row.ops[1])


def test_table_is_exactly_the_required_rows():
    keys = [key_of(r) for r in ROWS]
    assert len(set(keys)) == len(keys) == len({r.id for r in ROWS})
    req = required()
    assert len(req) == 2 * 24 + 27 + 13
    assert not req - set(keys), sorted(req - set(keys), key=str)[:5]
    assert not set(keys) - req, sorted(set(keys) - req, key=str)[:5]
    for row in ROWS:
        # class 0 is `plain` without and `act` with a pre-activation; knobs as the table's docstring says
        assert (row.ops[0] == "act") == (EPI_CLASS[row.ops[0]] == 0 and row.ops[1] >= 1), row.id
        if row.family == "wx4":
            r = str(row.emit_rows)
            assert row.env == {"VIRNET_CONV_FORM": "wx4", "VIRNET_WX4_MIN_TILES": "0", "VIRNET_WX4_MIN_COUT": "0", "VIRNET_WX4_MIN_FILL": "0",
                               "VIRNET_WX4_ROWS": r, "VIRNET_WX4_EMIT_ROWS": r, "VIRNET_WX4_NREP": row.env["VIRNET_WX4_NREP"]}, row.id
            assert row.single == dict(row.env, VIRNET_WX4_NREP="1"), row.id
        else:
            assert row.env == {"VIRNET_CONV_FORM": "f16x3" if row.family == "f16" else "bf16"}, row.id
