"""One table of the instantiations and plan edges of the f16-pipe weight gradient (csrc/wgrad_f16.hip): which call must run which
conv_wgrad_f16_kernel<NWV, BF, KG, S, DXM> under which split of the pixel range.  tests/test_wgrad_coverage.py (CPU) holds the table to
virnet_conv_wgrad_f16_plan_query, to the launchers' full set of instantiations and to the edge properties the rows are here for;
tests/test_wgrad_variants_gpu.py runs every row against an fp64 reference with the scratch poisoned.

Why pinned: every constant of the kernel (the row ring, the per-wave piece lists, the literal vmcnt, the accumulator tiles shared between
wave pairs, the three-row priming of a run) is a function of the template arguments, and which arguments a call gets follows from its
shape alone (make_plan: kg = 2 for w <= 32 else 4, nwv = min(3, output blocks)).  No knob is involved, so a row is just a shape.

mode 0: stride-1 3x3 (S=1, DXM=7), ops.conv_wgrad.  x [n, cx, h, w], dy [n, cy, h, w]; the real channels are the first cin / cout.
mode 1: 3x3 stride-2 conv (S=2, DXM=3), ops.conv_wgrad(stride=2).  (h, w) is the LOW-resolution size: x [n, cx, 2h, 2w], dy [n, cy, h, w].
mode 2: 2x2 transposed conv (S=2, DXM=2), ops.convt_wgrad.  (h, w) is the LOW-resolution size: x [n, cx, h, w], dy [n, cy, 2h, 2w].
The kernel's output-channel side (NWV) is dy for modes 0 and 1 and x for mode 2; query_args() gives the plan query's arguments.
pre: the staging transform of x -- 0 none, 1 LeakyReLU(0.2), 2 x * in_mul + in_add, then LeakyReLU(0.2).  bf16 rows take 0 or 1 (the fused
multiply-add's last bit can move a bf16 rounding, which no reference reproduces); the transposed conv has none.
plan: the (kg, nwv, split, run, nsteps) the row must get.

Pure data: no torch, no device."""
from collections import namedtuple

S1, S2, CONVT = range(3)                                   # virnet_conv_wgrad_f16_plan_query's mode
MODE_NAME = {S1: "s1", S2: "s2", CONVT: "convt"}

Row = namedtuple("Row", "id mode bf16 cin cout cx cy n h w bias_channels pre plan")


def _row(tag, mode, bf16, cin, cout, n, h, w, plan, *, cx=None, cy=None, bias=None, pre=0):
    cx, cy = cin if cx is None else cx, cout if cy is None else cy
    rid = f"{tag}-{MODE_NAME[mode]}-{'bf16' if bf16 else 'f16'}-c{cin}to{cout}-n{n}h{h}w{w}"
    return Row(rid, mode, bf16, cin, cout, cx, cy, n, h, w, cout if bias is None else bias, pre, plan)


def query_args(row):
    """(n, h, w, cx, cy, mode) of virnet_conv_wgrad_f16_plan_query: modes 1 / 2 take the stored channels of the high- / low-resolution operand"""
    hi_lo = {S1: (row.cx, row.cy), S2: (row.cx, row.cy), CONVT: (row.cy, row.cx)}[row.mode]
    return (row.n, row.h, row.w, *hi_lo, row.mode)


def out_blocks(row):
    """32-channel blocks on the kernel's output-channel side, in blocks on the other (both column phases for the stride-2 forms)"""
    _, _, _, a, b, mode = query_args(row)
    return (b + 31) // 32, ((a + 31) // 32 if mode == S1 else 2 * (a // 32))


def _instantiation_rows():
    """One row per (mode, BF, KG, NWV), at the smallest shapes the ABI takes: two images, 5..9 rows, one narrow strip (KG=2) or a
    64-pixel strip and a second one of one or two pixels (KG=4).  The heights rotate so that the number of runs takes every value mod 4
    within the stride-1 rows and within the stride-2 / transposed rows.  nsteps = 2h (KG=2) or 4h (KG=4); split = nsteps // 4."""
    rows = []
    for mode in (S1, S2, CONVT):
        for bf in (0, 1):
            for kg in (2, 4):
                for nwv in (1, 2, 3):
                    h = 5 + (nwv - 1 + 3 * bf + mode) % 5
                    w = (32, 23, 9)[nwv - 1] if kg == 2 else 65 + bf
                    wide, narrow = 32 * nwv, 32
                    cin, cout = (wide, narrow) if mode == CONVT else (narrow, wide)
                    nsteps = 2 * h * (1 if kg == 2 else 2)
                    split = nsteps // 4
                    pre = 0 if mode == CONVT else (nwv + kg // 2) % (2 if bf else 3)
                    rows.append(_row(f"kg{kg}nwv{nwv}", mode, bf, cin, cout, 2, h, w, (kg, nwv, split, -(-nsteps // split), nsteps), pre=pre))
    return rows


def _edge_rows():
    return [
        # empty trailing runs: split is capped at nsteps // 4 only, so split * run can pass nsteps by more than a run.  21 pairs -> split 12 of
        # 50 steps, runs of 5: runs 10 and 11 have no step and must still leave zeros in their scratch slices
        _row("empty2", S1, 0, 224, 288, 2, 25, 64, (4, 3, 12, 5, 50), pre=1),
        _row("empty1", S2, 0, 32, 32, 1, 25, 16, (2, 1, 6, 5, 25), pre=1),
        _row("empty1", CONVT, 1, 96, 64, 2, 15, 16, (2, 3, 7, 5, 30)),
        # a single run (nothing to reduce), five steps: the shortest run there is
        _row("single", S1, 0, 96, 96, 1, 5, 64, (4, 3, 1, 5, 5), pre=2),
        _row("single", S2, 1, 32, 64, 1, 5, 32, (2, 2, 1, 5, 5)),
        # seventeen runs: one pass of the stride-1 reduction's sixteen-wide loop and one run in its tail
        _row("runs17", S1, 0, 32, 32, 2, 17, 65, (4, 1, 17, 4, 68)),
        # four and five output blocks: the second three-block group is two / one short (`active`, the min(.., ncob - 1) clamp)
        _row("ncob4", S1, 0, 32, 128, 2, 6, 20, (2, 3, 3, 4, 12), pre=1),
        _row("ncob5", S1, 1, 32, 160, 2, 5, 65, (4, 3, 5, 4, 20)),
        _row("ncob4", S2, 1, 32, 128, 2, 7, 66, (4, 3, 7, 4, 28), pre=1),
        _row("ncob5", CONVT, 0, 160, 32, 2, 6, 12, (2, 3, 3, 4, 12)),
        # partial channel blocks (stride 1): 40 stored channels = a quarter-full second block; the tail conv's record shapes, 4 / 3 real channels of
        # 16 stored ones (the test fills the others with junk of order 1e3)
        _row("cin40", S1, 0, 40, 32, 2, 7, 30, (2, 1, 3, 5, 14), pre=2),
        _row("record", S1, 0, 4, 3, 2, 9, 66, (4, 1, 9, 4, 36), cx=16, cy=16, bias=3, pre=1),
        _row("record", S1, 0, 96, 3, 2, 8, 33, (4, 1, 4, 4, 16), cy=16, bias=3),
    ]


ROWS = _instantiation_rows() + _edge_rows()
BY_ID = {r.id: r for r in ROWS}


def reached(row):
    """(mode, BF, KG, NWV): the template arguments the row's launch switches on"""
    return (row.mode, row.bf16, row.plan[0], row.plan[1])
