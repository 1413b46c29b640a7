"""Every multi-slab instantiation of the split-fp16 convolution hosts (tests/variant_cases.py) on the device.  Per row:
  (a) what ran is what the row records: virnet_conv_plan_query on the descriptor of the call itself (and virnet_conv_wx4_last_plan);
  (b) every stored tensor against an fp64 convolution with the whole epilogue, at 2e-5 -- the bar tests/test_conv_f16_gpu.py and
      tests/test_conv_wx4_gpu.py hold the same kernels to on the same data (make_conv / rnd: O(1) activations, outputs of O(1));
  (c) the same call with the single-slab grouping gives the same bits (conv_plan.h: "No result bit depends on the grouping").
An error in the second or third slab's weight staging, bias / inverse-scale lookup, slab_base offset or epilogue turn-around fails (b) in
that slab's 32 channels and (c) with it; the small default shapes of the older kernel-level files never get that far (they plan NREP = 1).
bf16 rows: the reference takes bf16-rounded operands, as test_bf16_operand_variant_is_exactly_bf16_rounded_operands does."""
import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import make_conv, nchw, nhwc, rnd
from test_redzone_gpu import Launches
from variant_cases import BY_ID, RANGE_GUARD, ROWS
from virnet_amd import _native as nat
from virnet_amd import ops

pytestmark = pytest.mark.gpu
TOL = 2e-5
KNOBS = ("VIRNET_DETERMINISTIC", "VIRNET_WINOGRAD", "VIRNET_WX4_ROWS", "VIRNET_WX4_NREP", "VIRNET_WX4_WIDE", "VIRNET_WX4_PERSIST", "VIRNET_WX4_MIN_WGS",
         "VIRNET_WX4_MIN_TILES", "VIRNET_WX4_MIN_COUT", "VIRNET_WX4_MIN_FILL", "VIRNET_F16_SPLIT_WGS", "VIRNET_F16_MREP", "VIRNET_S2_SPLIT_TILES",
         "VIRNET_CONVT_KS", "VIRNET_CONVT_SLABS", "VIRNET_CONV_FORM")
LAUNCH = ("form", "rows", "ng", "nrep", "variant", "slab_base", "groups", "persistent")
FAMILY = {"wx4": nat.PLAN_WX4, "f16": nat.PLAN_F16, "bf16": nat.PLAN_BF16, "s2": nat.PLAN_F16, "convt": nat.PLAN_F16}
TIMER_NAME = {"wx4": "wx4", "f16": "f16x3", "bf16": "bf16", "s2": "f16x3_s2", "convt": "f16x3_t"}


def setenv(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def lrelu64(t, slope):
    return torch.where(t > 0, t, t * slope)


class Case:
    """The tensors of a row (built once), the call on them and the fp64 reference of everything the call stores."""

    def __init__(self, row, poke=None):
        self.row = row
        n, h, w, cin, cout = row.n, row.h, row.w, row.cin, row.cout
        fam = row.family
        self.cp = make_conv(cin, cout, **{"s2": dict(stride=2), "convt": dict(ks=2, stride=2, transposed=True)}.get(fam, {}), seed=80)
        self.x = rnd(n, cin, h, w, seed=81)
        if poke is not None:
            self.x[0, 70, h // 2, w // 2] = poke
        oh, ow = {"s2": (h // 2, w // 2), "convt": (2 * h, 2 * w)}.get(fam, (h, w))
        self.res, self.mask = rnd(n, cout, oh, ow, seed=82), rnd(n, cout, oh, ow, seed=83)
        self.imul, self.iadd = rnd(n, cin, seed=84, lo=0.3, hi=1.0), rnd(n, cin, seed=85)
        self.omul, self.oadd = rnd(n, cout, seed=86, lo=0.3, hi=1.0), rnd(n, cout, seed=87)
        self.wt, self.bias = self.cp.weight.detach().clone(), self.cp.bias.detach().clone()
        self.cp.cuda()
        self.dev = {k: (nhwc(getattr(self, k)) if getattr(self, k).dim() == 4 else getattr(self, k).cuda()) for k in ("x", "res", "mask", "imul", "iadd", "omul", "oadd")}

    def calls(self):
        """[(stride, keyword arguments of ops.conv_mfma)]: one call, or the raw and the activated store of the single-store hosts"""
        d, fam = self.dev, self.row.family
        if fam == "s2":
            return [(2, dict(want_raw=True)), (2, dict(want_raw=False, want_act=True, slope=0.2))]
        if fam == "convt":
            kw = dict(res=d["res"]) if self.row.ops[0] else {}
            return [(1, dict(kw, want_raw=True)), (1, dict(kw, want_raw=False, want_act=True, slope=0.2))]
        epi, pre = self.row.ops
        kw = {"plain": dict(want_raw=True), "act": dict(want_raw=False, want_act=True, slope=0.25), "res": dict(res=d["res"], want_raw=True),
              "mask": dict(mask=d["mask"], mask_slope=0.2, want_raw=True), "mask_res": dict(mask=d["mask"], mask_slope=0.2, res=d["res"], want_raw=True),
              "dual": dict(res=d["res"], want_raw=True, want_act=True, slope=0.25),
              "sft": dict(res=d["res"], mul=d["omul"], add=d["oadd"], want_raw=True, want_act=True, slope=0.25)}[epi]
        if pre >= 1:
            kw["in_slope"] = 0.2
        if pre == 2:
            kw.update(in_mul=d["imul"], in_add=d["iadd"])
        return [(1, kw)]

    def run(self):
        """-> (stored tensors, NHWC on the device; the Launches record; the launch timer's names)"""
        out = []
        with Launches() as rec:
            for stride, kw in self.calls():
                out += [t for t in ops.conv_mfma(self.dev["x"], self.cp.packed(), stride=stride, **kw) if t is not None]
            names = rec.names()
        return out, rec, names

    def reference(self):
        """fp64, NCHW, in the order run() returns the stored tensors"""
        n, cin, cout, fam = self.row.n, self.row.cin, self.row.cout, self.row.family
        wt, b = self.wt.double(), self.bias.double()
        if fam == "s2":
            y = F.conv2d(self.x.double(), wt, b, stride=2, padding=1)
            return [y, lrelu64(y, 0.2)]
        if fam == "convt":
            y = F.conv_transpose2d(self.x.double(), wt, b, stride=2)
            if self.row.ops[0]:
                y = y + self.res.double()
            return [y, lrelu64(y, 0.2)]
        epi, pre = self.row.ops
        if fam == "bf16":                                  # operands as the kernel sees them: fp32 LeakyReLU, then bf16 rounding of input and weight
            a = bf16_round(F.leaky_relu(self.x, 0.2) if pre == 1 else self.x).double()
            wt = bf16_round(self.wt).double()
        else:
            a = self.x.double()
            if pre == 2:
                a = a * self.imul.double().view(n, cin, 1, 1) + self.iadd.double().view(n, cin, 1, 1)
            if pre >= 1:
                a = lrelu64(a, 0.2)
        y = F.conv2d(a, wt, b, padding=1)
        if epi in ("mask", "mask_res"):
            y = y * torch.where(self.mask > 0, 1.0, 0.2).double()
        if epi in ("res", "mask_res", "dual", "sft"):
            y = y + self.res.double()
        if epi == "act":
            return [lrelu64(y, 0.25)]
        if epi == "dual":
            return [y, lrelu64(y, 0.25)]
        if epi == "sft":
            return [y, lrelu64(y * self.omul.double().view(n, cout, 1, 1) + self.oadd.double().view(n, cout, 1, 1), 0.25)]
        return [y]


def planned(rec, family):
    return [[tuple(l[k] for k in LAUNCH) for l in ops.conv_plan_query(FAMILY[family], d)] for d, _, _ in rec.convs]


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_variant_against_fp64_and_single_slab_grouping(monkeypatch, row):
    case = Case(row)
    refs = case.reference()
    # (a) + (b) under the row's knobs
    setenv(monkeypatch, row.env)
    outs, rec, names = case.run()
    assert names == [TIMER_NAME[row.family]], names
    plans = planned(rec, row.family)
    assert plans and all(p == row.launches for p in plans), (plans, row.launches)
    if row.family == "wx4":
        first = row.launches[0]
        assert ops.wx4_last_plan() == {"rows": first[1], "persistent": False, "slabs": first[3], "launches": len(row.launches)}
    assert len(outs) == len(refs)
    errs = [float((nchw(o).double() - r).abs().max()) for o, r in zip(outs, refs)]
    print(f"{row.id}: max error against fp64 {errs}")
    assert all(tuple(nchw(o).shape) == tuple(r.shape) for o, r in zip(outs, refs))
    assert all(e <= TOL for e in errs), errs
    # (c) the single-slab grouping: the same bits
    setenv(monkeypatch, row.single)
    singles, rec1, _ = case.run()
    plans1 = planned(rec1, row.family)
    assert plans1 and all(p == row.single_launches for p in plans1), (plans1, row.single_launches)
    for i, (o, s) in enumerate(zip(outs, singles)):
        assert torch.equal(o, s), (i, float((o - s).abs().max()))


@pytest.mark.parametrize("form", ["wx4", "f16x3"])
def test_deterministic_switch_makes_image_0_independent_of_the_batch(monkeypatch, form):
    """VIRNET_DETERMINISTIC=1 at 96 channels, 64 x 96: the slab grouping still follows the batch size (plan_wx4's `want`: one slab per
    workgroup for 1 and 2 images, three for 5 on 256 CUs; plan_f16's split_below likewise) -- image 0 must not notice."""
    setenv(monkeypatch, {"VIRNET_DETERMINISTIC": "1", "VIRNET_CONV_FORM": form})
    c, h, w = 96, 64, 96
    cp = make_conv(c, c, seed=80).cuda()
    x, res = rnd(5, c, h, w, seed=81), rnd(5, c, h, w, seed=82)
    outs, slabs = {}, {}
    for n in (1, 2, 5):
        with Launches() as rec:
            raw, act = ops.conv_mfma(nhwc(x[:n]), cp.packed(), in_slope=0.2, res=nhwc(res[:n]), want_raw=True, want_act=True, slope=0.25)
            assert rec.names() == [form]
        outs[n] = (raw[0].clone(), act[0].clone())
        slabs[n] = [l["nrep"] for d, _, _ in rec.convs for l in ops.conv_plan_query(FAMILY["wx4" if form == "wx4" else "f16"], d)]
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert slabs == {1: [1], 2: [1], 5: [3]}, slabs
    for n in (2, 5):
        assert torch.equal(outs[n][0], outs[1][0]) and torch.equal(outs[n][1], outs[1][1]), (n, slabs)


@pytest.mark.parametrize("rid,over,under", RANGE_GUARD, ids=[g[0] for g in RANGE_GUARD])
def test_range_guard_in_the_three_slab_forms(monkeypatch, rid, over, under):
    """The sticky range flag (virnet_set_range_flag) from the NREP=3 instantiations: an operand beyond fp16's range at input channel 70
    raises it, one below does not."""
    row = BY_ID[rid]
    setenv(monkeypatch, row.env)
    dev = torch.device("cuda", torch.cuda.current_device())
    flag = ops.range_flag(dev)
    assert flag is not None
    flag.zero_()
    for amp, expect in ((under, False), (over, True)):
        case = Case(row, poke=amp)
        _, rec, _ = case.run()
        assert all(p == row.launches for p in planned(rec, row.family))
        assert ops.range_overflowed(dev) is expect, (rid, amp)
    assert not ops.range_overflowed(dev)
