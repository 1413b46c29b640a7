"""ops.conv_form_rule -- which kernel family conv_mfma launches and the tile height it emits with -- against a table recorded from the
commit before the rule was a function one can call: tests/golden/conv_forms.json (tests/golden/make_conv_forms.py says how it was
recorded, and from what).  CPU only: the rule takes plain values and reads the knobs."""
import itertools
import json
import os

from virnet_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("VIRNET_CONV_FORM", "VIRNET_WINOGRAD", "VIRNET_DETERMINISTIC", "VIRNET_WX4_MIN_WGS", "VIRNET_WX4_MIN_COUT", "VIRNET_WX4_MIN_FILL",
         "VIRNET_WX4_MIN_TILES", "VIRNET_WX4_MIN_SLAB_WGS", "VIRNET_WX4_ROWS", "VIRNET_WX4_EMIT_ROWS", "VIRNET_T_EMIT")


def table():
    """the table with its lines spelled out as rows: [layer, images, n, h, w, operands, want, emit, knobs, form, emit rows]"""
    with open(os.path.join(ROOT, "tests", "golden", "conv_forms.json")) as f:
        tab = json.load(f)
    forms = {v: k for k, v in tab["codes"].items()}
    tab["rows"] = [spec[:7] + [emit, knobs, forms[res[0]], int(res[1:])] for spec in tab["specs"]
                   for (emit, knobs), res in zip(itertools.product(tab["emits"], tab["knobs"]), spec[7].split(" "), strict=True)]
    return tab


def rule_of(row, layer, environ, scoped=False):
    """the rule's answer for a table row under the row's knobs; ``layer``: (transposed, stride, c, cout, stored channels); ``scoped``: asked
    as the engine asks, inside a forward_scope (knobs from its snapshot, thresholds parsed once)"""
    _, images, n, h, w, operands, want, emit, knobs = row[:9]
    transposed, stride, c, cout, cstore = layer
    for k in KNOBS:
        environ.pop(k, None)
    environ.update(knobs)
    images, operands = images.split("+"), operands.split("+")
    args = ("wino" in images, "f16" in images, "bf16" in images, "wx4" in images, bool(transposed), stride, cstore == cout,
            n, h, w, c, cout, "res" in operands, "mask" in operands, "mul" in operands, "in_mul" in operands,
            want in ("raw", "both"), want in ("act", "both"), emit != 0)
    if scoped:
        with ops.forward_scope():
            return ops.conv_form_rule(*args)
    return ops.conv_form_rule(*args)


def differing(tab, scoped):
    layers = {k: tuple(v[f] for f in ("transposed", "stride", "c", "cout", "cstore")) for k, v in tab["layers"].items()}
    before = {k: os.environ.get(k) for k in KNOBS}
    try:
        return [(row, got) for row in tab["rows"] for got in [rule_of(row, layers[row[0]], os.environ, scoped)] if list(got) != row[9:11]]
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_table_covers_every_branch_and_knob():
    tab = table()
    rows = tab["rows"]
    assert 2000 <= len(rows)
    assert {r[9] for r in rows} == {"direct", "wino", "f16x3", "bf16", "wx4"} and {r[10] for r in rows} == {0, 8, 16}
    assert {k for r in rows for k in r[8]} == set(KNOBS) and {r[7] for r in rows} == {0, 1, 2} and {r[2] for r in rows} == {1, 4, 6, 32}
    assert {r[8].get("VIRNET_WX4_MIN_WGS") for r in rows} == {None, "0", "64", "100000"}
    assert {r[8].get("VIRNET_CONV_FORM") for r in rows} == {None, "wx4", "f16x3", "wino", "direct", "bf16"}
    assert all(v > 0 for v in tab["branch_hits"].values()) and len(tab["branch_hits"]) >= 30
    # the launch that shows the emission's own bound: 4 x 64 x 64 x 160 channels = 64 workgroups take the Winograd form under
    # VIRNET_WX4_MIN_WGS=64 (not under the default), and the emitting launch still leaves it -- its bound of 128 does not follow the knob
    shown = [r for r in rows if r[:6] == ["cc160", "f16+wx4", 4, 64, 64, ""]]
    assert {(r[7], r[9]) for r in shown if r[8] == {"VIRNET_WX4_MIN_WGS": "64"}} == {(0, "wx4"), (1, "f16x3"), (2, "f16x3")}
    assert {(r[7], r[9]) for r in shown if r[8] == {}} == {(0, "f16x3"), (1, "f16x3"), (2, "f16x3")}


def test_rule_reproduces_the_recorded_forms():
    tab = table()
    bad = differing(tab, scoped=False)
    assert not bad, f"{len(bad)} of {len(tab['rows'])} rows differ, first: {bad[:3]}"


def test_rule_reproduces_them_inside_a_forward_scope():
    tab = table()
    bad = differing(tab, scoped=True)
    assert not bad, f"{len(bad)} of {len(tab['rows'])} rows differ, first: {bad[:3]}"
