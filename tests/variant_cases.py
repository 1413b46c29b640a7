"""One table of the multi-slab instantiations of the split-fp16 convolution hosts (csrc/conv_plan.h): which call, under which knobs,
must run which launches.  tests/test_variant_coverage.py (CPU) holds the table to virnet_conv_plan_query and to the dispatch code's full
set of instantiations; tests/test_conv_variants_gpu.py runs every row against an fp64 reference and against the single-slab grouping.

Why pinned: the plan rules for under-filled launches (plan_wx4's `want`, plan_f16's split_below, plan_f16_s2's s2_split_tiles) give every
small test shape ONE 32-channel slab per workgroup, so a kernel-level test at a small shape never runs NREP >= 2 unless a knob says so.
Every row pins its variant with knobs that make the plan independent of the CU count:
  wx4 / wx4h   VIRNET_WX4_ROWS=16|8 + VIRNET_WX4_NREP=3|2 (unset at 160 channels / 8 rows: the five-slab form), the four VIRNET_WX4_MIN_*=0
  f16 / bf16   VIRNET_F16_SPLIT_WGS=0 + VIRNET_F16_MREP=1|2
  s2           VIRNET_S2_SPLIT_TILES=0
  convt        VIRNET_CONVT_KS=3, VIRNET_CONVT_SLABS=3
`single` is the environment of the same call with the smallest slab grouping (VIRNET_WX4_NREP=1, VIRNET_F16_SPLIT_WGS=100000,
VIRNET_S2_SPLIT_TILES=100000; transposed: VIRNET_CONVT_SLABS=2, and KS=2 instead of KS=3 where the contraction length allows both):
channels are independent, so it must give the same bits.

Shapes: the smallest with a partial tile on both axes and a second image, n=2, h=tile rows+1, w=33, unless a row says otherwise.

Pure data: no device."""
from collections import namedtuple

from virnet_amd import _native

# virnet_conv_launch.form
WX4, WX4H, WX4P, F16, S2, CONVT = (_native.LAUNCH_WX4, _native.LAUNCH_WX4H, _native.LAUNCH_WX4P, _native.LAUNCH_F16, _native.LAUNCH_S2,
                                   _native.LAUNCH_CONVT)
FORM_NAME = {WX4: "wx4", WX4H: "wx4h", F16: "f16", S2: "s2", CONVT: "convt"}

# family: wx4 | f16 | bf16 | s2 | convt.  ops: the operand set -- stride 1: (epilogue, pre); s2: (); convt: (bridge,).
# launches: [(form, rows, ng, nrep, variant, slab_base, groups, persistent)] under `env`; single_launches: the same under `single`.
Row = namedtuple("Row", "id family n h w cin cout ops env launches single single_launches")

# epilogue class (conv_plan.h epi_of) -> the operand sets that spell it; a row takes the first at 96 channels, the second elsewhere
#   plain: y_raw | act: y_act only | res: residual | mask | mask_res | dual: residual + both stores | sft: dual + output mul / add
EPI = {0: ("plain", "act"), 1: ("res", "res"), 2: ("mask", "mask"), 3: ("mask_res", "mask_res"), 4: ("sft", "dual")}
EPI_CLASS = {name: cls for cls, names in EPI.items() for name in names}
# pre-activation class (pre_of): 0 none, 1 LeakyReLU (in_slope), 2 SFT (in_mul / in_add + in_slope)

_WX4_OPEN = {"VIRNET_CONV_FORM": "wx4", "VIRNET_WX4_MIN_TILES": "0", "VIRNET_WX4_MIN_COUT": "0", "VIRNET_WX4_MIN_FILL": "0", "VIRNET_WX4_MIN_WGS": "0"}

# slabs per workgroup x channel blocks, written out per channel count (conv_plan.h slab_groups: 3 where the count allows, the rest in 2s)
GROUPS3 = {64: [(2, 1)], 96: [(3, 1)], 128: [(2, 2)], 160: [(3, 1), (2, 1)], 192: [(3, 2)], 224: [(3, 1), (2, 2)], 288: [(3, 3)]}


def _launches(form, rows, variant, groups):
    out, base = [], 0
    for nrep, g in groups:
        out.append((form, rows, 1, nrep, variant, base, g, 0))
        base += nrep * g
    return out


def _s1_ops(cout, cls, pre):
    return (EPI[cls][0 if cout == 96 else 1], pre)


def _wx4_rows():
    rows = []
    for r in (16, 8):
        form, shape = (WX4 if r == 16 else WX4H), (2, r + 1, 33)
        env3 = dict(_WX4_OPEN, VIRNET_WX4_ROWS=str(r), VIRNET_WX4_NREP="3")
        single = dict(env3, VIRNET_WX4_NREP="1")

        def row(tag, cin, cout, ops, env, groups):
            rows.append(Row(f"wx4-r{r}-{tag}-{ops[0]}-pre{ops[1]}", "wx4", *shape, cin, cout, ops, env, _launches(form, r, 0, groups),
                            single, _launches(form, r, 0, [(1, cout // 32)])))
        # every epilogue class x every pre-activation class on the three-slab (96) and the two-slab (64) workgroup
        for c in (96, 64):
            for cls in range(5):
                for pre in range(3):
                    row(f"c{c}", c, c, _s1_ops(c, cls, pre), env3, GROUPS3[c])
        # the mixed groupings (second / third launch at slab_base 3 / 5), three channel blocks, an odd chunk count; NREP=2 pinned on 192
        for i, (cin, cout) in enumerate([(160, 160), (224, 224), (288, 288), (48, 96)]):
            row(f"c{cin}to{cout}", cin, cout, _s1_ops(cout, i % 5, i % 3), env3, GROUPS3[cout])
        row("c192-nrep2", 192, 192, _s1_ops(192, 4, 1), dict(env3, VIRNET_WX4_NREP="2"), [(2, 3)])
    # 160 channels on 8-row tiles without VIRNET_WX4_NREP: ONE launch of the five-slab form (conv_wx4h_kernel<5, EPI, PRE>)
    env5 = dict(_WX4_OPEN, VIRNET_WX4_ROWS="8")
    for cls in range(5):
        for pre in range(3):
            ops = _s1_ops(160, cls, pre)
            rows.append(Row(f"wx4-r8-c160-nrep5-{ops[0]}-pre{pre}", "wx4", 2, 9, 33, 160, 160, ops, env5, [(WX4H, 8, 1, 5, 0, 0, 1, 0)],
                            dict(env5, VIRNET_WX4_NREP="1"), _launches(WX4H, 8, 0, [(1, 5)])))
    return rows


def _f16_rows():
    rows = []
    for m in (1, 2):
        shape = (2, 4 * m + 1, 33)
        for family in ("f16", "bf16"):
            env = {"VIRNET_CONV_FORM": "f16x3" if family == "f16" else "bf16", "VIRNET_F16_SPLIT_WGS": "0", "VIRNET_F16_MREP": str(m)}
            single = dict(env, VIRNET_F16_SPLIT_WGS="100000")

            def row(tag, cin, cout, ops, groups):
                rows.append(Row(f"{family}-m{m}-{tag}-{ops[0]}-pre{ops[1]}", family, *shape, cin, cout, ops, env, _launches(F16, 4 * m, m, groups),
                                single, _launches(F16, 4 * m, m, [(1, cout // 32)])))
            # every epilogue class on the three-slab and the two-slab workgroup.  The pre-activation is a run-time branch of this kernel
            # (no template parameter): f16 takes each class with none / in_slope / in_mul; bf16 rounds the pre-activated input to bf16, which
            # a reference can reproduce for the LeakyReLU (one fp32 product) and not for the SFT's fp32 multiply-add, so bf16 alternates 0 / 1
            for c in (96, 64):
                for cls in range(5):
                    for pre in (range(3) if family == "f16" else [cls % 2]):
                        row(f"c{c}", c, c, _s1_ops(c, cls, pre), GROUPS3[c])
            others = [(128, 128), (160, 160), (224, 224), (288, 288), (48, 96)] if family == "f16" else [(160, 160)]
            for i, (cin, cout) in enumerate(others):
                row(f"c{cin}to{cout}", cin, cout, _s1_ops(cout, (i + m) % 5, (i + m) % (3 if family == "f16" else 2)), GROUPS3[cout])
    return rows


def _s2_rows():
    env = {"VIRNET_CONV_FORM": "f16x3", "VIRNET_S2_SPLIT_TILES": "0"}
    single = dict(env, VIRNET_S2_SPLIT_TILES="100000")
    small = (2, 10, 66)                                    # INPUT size: 5 x 33 outputs, 2 x 2 tiles of 4 x 32 per image
    cases = [("wide4", small, 96, 128, [(S2, 4, 1, 4, 0, 0, 1, 0)]),
             ("wide5", small, 96, 160, [(S2, 4, 1, 5, 0, 0, 1, 0)]),
             ("wide7", small, 160, 224, [(S2, 4, 1, 7, 0, 0, 1, 0)]),
             ("g3x2", small, 96, 192, [(S2, 4, 1, 3, 0, 0, 2, 0)]),                                # six slabs below 192 tiles: <1,3>, two groups
             ("g2", small, 64, 64, [(S2, 4, 1, 2, 0, 0, 1, 0)]),
             # 6 x 16 x 2 = 192 tiles of 4 x 32: exactly where the 8-wave form starts; 9 slabs = <2,3> + <1,3> at slab 6
             ("g6g3", (6, 122, 66), 48, 288, [(S2, 4, 2, 3, 0, 0, 1, 0), (S2, 4, 1, 3, 0, 6, 1, 0)])]
    return [Row(f"s2-{tag}-c{cin}to{cout}", "s2", *shape, cin, cout, (), env, launches, single, [(S2, 4, 1, 1, 0, 0, cout // 32, 0)])
            for tag, shape, cin, cout, launches in cases]


def _convt_rows():
    # The pointwise GEMM has 4 * cout / 32 = cout / 8 slabs, a multiple of 4: slab_groups6 gives 6s and 2s for every such count (4 = 2 + 2,
    # 8 = 6 + 2, 20 = 6 + 6 + 6 + 2, 24 = 6 x 4).  <1,3> needs VIRNET_CONVT_SLABS=3 (8 = 3 + 3 + 2), and NO knob value plans <1,1>: launch_f16_convt's
    # last branch cannot be reached through plan_f16_convt.
    # The packing accepts every cin % 16 == 0: 48 pads its contraction to 48 (KS=3 only, no knob), 80 to 96 (KS=2 by default with a
    # zero sixth chunk, KS=3 with the knob: a zero-padded second stage).
    rows = []
    shape = (2, 5, 33)                                     # 330 pixels: two 128-pixel tiles and a partial one
    g6 = lambda ks, cout: {192: [(2, 3, 0, 4)], 160: [(2, 3, 0, 3), (1, 2, 18, 1)], 64: [(2, 3, 0, 1), (1, 2, 6, 1)], 32: [(1, 2, 0, 2)]}[cout]
    cases = [("ks2", 96, 192, {}, 2, None),                # (the production form <2,3,KS=2>, so that the table holds the whole dispatch set)
             ("ks3", 96, 192, {"VIRNET_CONVT_KS": "3"}, 3, None), ("ks3", 192, 160, {"VIRNET_CONVT_KS": "3"}, 3, None),
             ("ks3", 288, 64, {"VIRNET_CONVT_KS": "3"}, 3, None), ("ks3", 96, 32, {"VIRNET_CONVT_KS": "3"}, 3, None),
             ("pad48", 48, 32, {}, 3, None), ("pad80", 80, 32, {}, 2, None), ("pad80-ks3", 80, 32, {"VIRNET_CONVT_KS": "3"}, 3, None),
             ("slabs3-ks3", 96, 64, {"VIRNET_CONVT_KS": "3", "VIRNET_CONVT_SLABS": "3"}, 3, [(1, 3, 0, 2), (1, 2, 6, 1)]),
             ("slabs3-ks2", 96, 64, {"VIRNET_CONVT_SLABS": "3"}, 2, [(1, 3, 0, 2), (1, 2, 6, 1)])]
    for tag, cin, cout, knobs, ks, groups in cases:
        env = dict(knobs, VIRNET_CONV_FORM="f16x3")
        kpad = cin if cin % 32 == 0 else (cin + 47) // 48 * 48          # (conv_plan.h convt_kpad)
        both = kpad % 96 == 0                                           # stages of two and of three chunks are both legal
        single_ks = (2 if ks == 3 else 3) if both else ks
        single = {"VIRNET_CONV_FORM": "f16x3", "VIRNET_CONVT_SLABS": "2"}
        if single_ks == 3 and cin != 48:
            single["VIRNET_CONVT_KS"] = "3"
        for bridge in (True, False):
            rows.append(Row(f"convt-{tag}-c{cin}to{cout}-{'bridge' if bridge else 'plain'}", "convt", *shape, cin, cout, (bridge,), env,
                            [(CONVT, 0, ng, nrep, ks, base, g, 0) for ng, nrep, base, g in (groups or g6(ks, cout))],
                            single, [(CONVT, 0, 1, 2, single_ks, 0, cout // 16, 0)]))
    return rows


ROWS = _wx4_rows() + _f16_rows() + _s2_rows() + _convt_rows()
BY_ID = {r.id: r for r in ROWS}

# range guard, per family in its NREP=3 form: (row id, amplitude that must raise the flag, amplitude that must not), the operand at input channel 70
# (of 96: the channel range of the third slab).  The Winograd form flags the TRANSFORMED value (coefficients up to 5).
RANGE_GUARD = [("wx4-r16-c96-plain-pre0", 3.0e4, 5.0e3), ("wx4-r8-c96-plain-pre0", 3.0e4, 5.0e3), ("f16-m1-c96-plain-pre0", 7.0e4, 3.0e4),
               ("f16-m2-c96-plain-pre0", 7.0e4, 3.0e4), ("s2-g3x2-c96to192", 7.0e4, 3.0e4), ("convt-ks3-c96to192-plain", 7.0e4, 3.0e4)]


def reached(row, launches=None, family=None):
    """(form, rows, ng, nrep, variant, epi, pre) of every launch of a row -- the template arguments its dispatch switches on.  epi / pre are
    None where the kernel takes them at run time (conv_f16: pre; stride 2 and transposed: both)."""
    family = family or row.family
    out = set()
    for form, rows, ng, nrep, variant, _, _, _ in (row.launches if launches is None else launches):
        if family == "wx4":
            out.add((FORM_NAME[form], rows, ng, nrep, variant, EPI_CLASS[row.ops[0]], row.ops[1]))
        elif family in ("f16", "bf16"):
            out.add((family, rows, ng, nrep, variant, EPI_CLASS[row.ops[0]], None))
        else:
            out.add((FORM_NAME[form], rows, ng, nrep, variant, None, None))
    return out
