"""One table of the T-EMITTING instantiations of the stride-1 3x3 convolution hosts (TE = 1: the epilogue also writes the channel-major
image the weight-gradient GEMM contracts over, and per-block channel sums): which call, under which knobs, must run which launches.
tests/test_t_emit_coverage.py (CPU) holds the table to virnet_conv_plan_query, to ops.conv_form_rule and to the dispatch code's full set of
72 emitting instantiations; tests/test_t_emit_variants_gpu.py runs every row against an fp64 reference, a host-side T image and, for the
Winograd rows, the single-slab grouping.  Rows are variant_cases.Row plus `emit_rows`; every row goes through ops.conv_mfma(emit=...).

Operand sets (variant_cases.EPI_CLASS) and what is emitted with them -- emit_mode():
  plain     (class 0, pre 0)   raw store                                    T of the stored tensor      channel sums
  act       (class 0, pre >= 1) activated store only, slope 0.25 (conv1 of a training step)  T of the stored tensor   NO channel sums
  res       (class 1)          raw store + residual (conv2)                 T = lrelu(stored, 0.2)      channel sums
  mask / mask_res (2 / 3)      the input-gradient types                     T of the stored tensor      channel sums

Winograd family (launch_wx4<NREP, EPI, PRE, 1> on 16-row tiles, launch_wx4h_t<NREP, EPI, PRE, 1> on 8-row tiles): h = 17, w = 33 and the
smallest n with n * ceil(h / 16) * ceil(w / 32) * ceil(cout / 96) >= ops.WX4_EMIT_MIN_WGS = 128 -- below it ops.conv_form_rule hands an
unpinned emission to the direct kernel, and a pinned one (VIRNET_WX4_MIN_WGS=0, VIRNET_DETERMINISTIC=1) always emits from 16-row tiles, so
this is the only way ops.conv_mfma reaches the 8-row emitting kernels.  Knobs: VIRNET_CONV_FORM=wx4, the three VIRNET_WX4_MIN_{TILES,COUT,
FILL}=0, VIRNET_WX4_ROWS = VIRNET_WX4_EMIT_ROWS = r, VIRNET_WX4_NREP=3 | 2; VIRNET_WX4_MIN_WGS and VIRNET_DETERMINISTIC stay unset.  `single`:
the same call with VIRNET_WX4_NREP=1 (the only road to the NREP = 1 emitting instantiations besides the 160-channel NREP=2 row, whose
fifth slab is a single-slab launch at slab_base 4).

Direct family (launch<2, NREP, EPI, BF, 1>): emission always runs 8-row tiles (MREP = 2) and never splits slabs, so VIRNET_CONV_FORM alone
pins the plan; n = 2, h = 9, w = 33.  No partner.  plain_env(): the knobs of the NON-emitting call with the same grouping.

All of the above have wide T rows (w = 33: 10 segments); the *-w31 rows are the narrow kind (w <= 32: 6 segments).

Pure data: no torch, no device."""
from collections import namedtuple

from variant_cases import EPI_CLASS, F16, FORM_NAME, GROUPS3, WX4, WX4H, Row, _launches

TRow = namedtuple("TRow", Row._fields + ("emit_rows",))

OPS = {0: "plain", 1: "res", 2: "mask", 3: "mask_res"}
GROUPS = {**GROUPS3, 32: [(1, 1)]}
T_SLOPE = 0.2                                              # LeakyReLU of the T image of a `res` row


def ops_of(cls, pre):
    return ("act" if cls == 0 and pre >= 1 else OPS[cls], pre)


def emit_mode(row):
    """-> the `emit` argument of ops.conv_mfma for a row"""
    name = row.ops[0]
    return dict(act=T_SLOPE if name == "res" else None, colsum=None if name == "act" else row.cout)


def plain_env(row):
    """the knobs under which the NON-emitting call runs the row's grouping and tile form"""
    return dict(row.env) if row.family == "wx4" else dict(row.env, VIRNET_F16_MREP="2", VIRNET_F16_SPLIT_WGS="0")


def wx4_n(w, cout):
    """smallest n with n * ceil(17 / 16) * ceil(w / 32) * ceil(cout / 96) >= 128"""
    per = 2 * ((w + 31) // 32) * ((cout + 95) // 96)
    return (128 + per - 1) // per


def _wx4_rows():
    rows = []
    for r in (16, 8):
        form = WX4 if r == 16 else WX4H
        env3 = {"VIRNET_CONV_FORM": "wx4", "VIRNET_WX4_MIN_TILES": "0", "VIRNET_WX4_MIN_COUT": "0", "VIRNET_WX4_MIN_FILL": "0",
                "VIRNET_WX4_ROWS": str(r), "VIRNET_WX4_EMIT_ROWS": str(r), "VIRNET_WX4_NREP": "3"}

        def row(tag, cin, cout, ops, groups, nrep="3", w=33):
            env = dict(env3, VIRNET_WX4_NREP=nrep)
            rows.append(TRow(f"wx4-r{r}-{tag}-{ops[0]}-pre{ops[1]}", "wx4", wx4_n(w, cout), 17, w, cin, cout, ops, env, _launches(form, r, 0, groups),
                             dict(env, VIRNET_WX4_NREP="1"), _launches(form, r, 0, [(1, cout // 32)]), r))
        # every (EPI, PRE) on the three-slab (96) and the two-slab (64) workgroup
        for c in (96, 64):
            for cls in range(4):
                for pre in range(2):
                    row(f"c{c}", c, c, ops_of(cls, pre), GROUPS[c])
        # mixed groupings (T rows and partial sums at slab_base 3 and 5), three channel blocks, an odd chunk count, cin != cout
        for i, (cin, cout) in enumerate([(160, 160), (224, 224), (288, 288), (48, 96), (192, 96)]):
            row(f"c{cin}to{cout}", cin, cout, ops_of(i % 4, i % 2), GROUPS[cout])
        # groups of two: three blocks of them; 160 = <2> x 2 at slab 0, then <1> x 1 at slab_base 4
        row("c192-nrep2", 192, 192, ops_of(2, 1), [(2, 3)], nrep="2")
        row("c160-nrep2", 160, 160, ops_of(1, 0), [(2, 2), (1, 1)], nrep="2")
        row("c96-w31", 96, 96, ops_of(1, 0), GROUPS[96], w=31)
    return rows


def _direct_rows():
    rows = []

    def row(family, tag, cin, cout, ops, w=33):
        env = {"VIRNET_CONV_FORM": "f16x3" if family == "f16" else "bf16"}
        rows.append(TRow(f"{family}-{tag}-{ops[0]}-pre{ops[1]}", family, 2, 9, w, cin, cout, ops, env, _launches(F16, 8, 2, GROUPS[cout]), None, None, 8))
    # f16: the pre-activation is a run-time branch -- none / LeakyReLU / SFT (in_mul: conv_form_rule sends every emitting SFT conv1 here)
    for cls in range(4):
        for pre in range(3):
            row("f16", "c96", 96, 96, ops_of(cls, pre))
    for c in (64, 32):
        for cls in range(4):
            row("f16", f"c{c}", c, c, ops_of(cls, cls % 3))
    for i, (cin, cout) in enumerate([(128, 128), (160, 160), (224, 224), (288, 288), (48, 96), (192, 96)]):
        row("f16", f"c{cin}to{cout}", cin, cout, ops_of(i % 4, i % 3))
    row("f16", "c96-w31", 96, 96, ops_of(1, 0), w=31)
    # bf16: a reference cannot reproduce the bf16 rounding of an fp32 SFT (variant_cases alternates 0 / 1 for the same reason)
    for c in (96, 64, 32):
        for cls in range(4):
            row("bf16", f"c{c}", c, c, ops_of(cls, cls % 2))
    row("bf16", "c160to160", 160, 160, ops_of(1, 1))
    return rows


ROWS = _wx4_rows() + _direct_rows()
BY_ID = {r.id: r for r in ROWS}


def reached(row, launches=None):
    """(form, tile rows, NREP, EPI, PRE | BF) of every launch of a row: the template arguments the emitting dispatch switches on (the
    Winograd hosts: PRE 0 | 1; launch_f16_planned: bf16 operands 0 | 1, its pre-activation is a run-time branch)"""
    last = row.ops[1] if row.family == "wx4" else int(row.family == "bf16")
    return {(FORM_NAME[form], rows, nrep, EPI_CLASS[row.ops[0]], last) for form, rows, _, nrep, _, _, _, _ in (row.launches if launches is None else launches)}
