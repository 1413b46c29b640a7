"""Every instantiation of the fp32 direct convolution (csrc/conv_mfma.hip; the table is tests/mfma_cases.py) on the device.  Per row:
  (a) the tile rule names the row's instantiation for the call itself: the launch timer's key, and virnet_conv_mfma_tile on the call's own
      descriptor under the call's environment.  Both are answers of pick_tile, the rule the launch runs; that the dispatch launches
      exactly the instantiation the rule names is held by tests/test_mfma_coverage.py (the VIRNET_CASE list matches on all five values);
  (b) every stored tensor against an fp64 convolution with the whole epilogue, at 2e-5 -- the bar tests/test_ops_gpu.py holds this kernel
      to on the same data (make_conv / rnd: O(1) activations, outputs of O(1)); exp(clamp(.)) in that file's relative form;
  (c) the same call as <KS, STRIDE, 1, 1> on the same tensors gives the same bits: every instantiation walks K in the same order per output
      element (chunk, tap, half-step, one fp32 MFMA chain), and the epilogue is per element.
An error in the second or later slab's weight staging (slab0, the ring's slot arithmetic), in the second row block's pixel fragments or
epilogue offsets, in the 8-wave tile's staging split or in a channel block's base fails (b) there and (c) with it; the small default
shapes of the older kernel-level files never get that far (pick_tile gives them <KS, STRIDE, 1, 1>)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from mfma_cases import CLAMP, CROP, P_OPS, ROWS
from test_ops_gpu import make_conv, nchw, nhwc, rnd
from test_redzone_gpu import Launches
from virnet_amd import _native as nat
from virnet_amd import ops

pytestmark = pytest.mark.gpu
TOL = 2e-5
KNOBS = ("VIRNET_CONV_FORM", "VIRNET_WINOGRAD", "VIRNET_FORCE_MREP", "VIRNET_FORCE_NREP", "VIRNET_FORCE_NW")
NCHW_OP = {"plain": nat.NCHW_PLAIN, "add": nat.NCHW_ADD, "expclamp": nat.NCHW_EXPCLAMP}


def setenv(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")


def lrelu64(t, slope):
    return torch.where(t > 0, t, t * slope)


class Case:
    """The tensors of a row (built once, on the CPU and on the device), the call on them and the fp64 reference of everything it stores.
    Construct it under the row's environment: the packing follows VIRNET_CONV_FORM."""

    def __init__(self, row):
        self.row = row
        n, h, w, cin, cout, s = row.n, row.h, row.w, row.cin, row.cout, row.seed
        if row.kind == "convt":
            self.cp = make_conv(cin, cout, ks=2, stride=2, transposed=True, seed=s)
            oh, ow = 2 * h, 2 * w
        elif row.kind == "dgemm":                           # the layer whose input gradient this GEMM is: cout -> cin / 4 channels
            self.cp = make_conv(cout, cin // 4, ks=2, stride=2, transposed=True, seed=s)
            oh, ow = h, w
        else:
            self.cp = make_conv(cin, cout, stride=row.stride, seed=s)
            oh, ow = h // row.stride, w // row.stride
        self.wt = self.cp.weight.detach().clone()
        self.bias = None if row.kind == "dgemm" else self.cp.bias.detach().clone()
        self.x = rnd(n, cin, h, w, seed=s + 1)
        self.cp.cuda()
        t = dict(x=nhwc(self.x))
        if row.kind == "planar":
            op, sf = P_OPS[row.ops]
            ch, cw = CROP(row)
            if op == "add":
                self.res = rnd(n, cout, ch // sf, cw // sf, seed=s + 2)
                t["res"] = self.res.cuda()
        else:
            if row.ops in ("bias_res", "mask_res", "bridge"):
                self.res = rnd(n, cout, oh, ow, seed=s + 2)
                t["res"] = nhwc(self.res)
            if row.ops in ("mask_res", "mask"):
                self.mask = rnd(n, cout, oh, ow, seed=s + 3)
                t["mask"] = nhwc(self.mask)
            if row.ops == "sft":                            # per-image vectors: another one for every image
                self.omul, self.oadd = rnd(n, cout, seed=s + 4, lo=0.3, hi=1.0), rnd(n, cout, seed=s + 5)
                t.update(mul=self.omul.cuda(), add=self.oadd.cuda())
            if row.ops == "in_sft":                         # add != 0: the border must see zeros AFTER the activation
                self.imul, self.iadd = rnd(n, cin, seed=s + 6, lo=0.3, hi=1.0), rnd(n, cin, seed=s + 7, lo=0.2, hi=1.0)
                t.update(in_mul=self.imul.cuda(), in_add=self.iadd.cuda())
        self.tensors = t

    def packing(self):
        return self.cp.packed_dgrad() if self.row.kind == "dgemm" else self.cp.packed()

    def call(self, x, **more):
        """-> the stored tensors, in the order reference() lists them"""
        row = self.row
        if row.kind == "planar":
            op, sf = P_OPS[row.ops]
            return [ops.conv_mfma_nchw(x, self.packing(), CROP(row), op=NCHW_OP[op], res_sf=sf, clamp=CLAMP, **more)]
        kw = {"plain": dict(want_raw=True), "act": dict(want_raw=False, want_act=True, slope=0.25), "dual": dict(want_raw=True, want_act=True, slope=0.25),
              "bias_res": dict(want_raw=True), "bridge": dict(want_raw=True), "mask_res": dict(want_raw=True, mask_slope=0.2),
              "mask": dict(want_raw=True, mask_slope=0.2), "sft": dict(want_raw=True, want_act=True, slope=0.25),
              "in_act": dict(want_raw=True, in_slope=0.2), "in_sft": dict(want_raw=True, in_slope=0.2)}[row.ops]
        return [t for t in ops.conv_mfma(x, self.packing(), stride=row.stride, **more, **kw) if t is not None]

    def run(self):
        """-> (stored tensors on the device, the launch timer's keys of the direct kernel, the tiles virnet_conv_mfma_tile reports)"""
        with Launches() as rec:
            out = self.call(**self.tensors)
            keys = [k for k in rec.timer.summary() if isinstance(k[0], int)]
            tiles = []
            for d, form, _ in rec.convs:
                v = (ctypes.c_int * 5)()
                nat.check(nat.load().virnet_conv_mfma_tile(ctypes.byref(d), ctypes.byref(v)), "conv_mfma_tile")
                tiles.append((form, tuple(v)))
        return out, keys, tiles

    def reference(self):
        """fp64, NCHW"""
        row = self.row
        n, cin, cout = row.n, row.cin, row.cout
        a, wt = self.x.double(), self.wt.double()
        b = None if self.bias is None else self.bias.double()
        if row.ops == "in_sft":
            a = a * self.imul.double().view(n, cin, 1, 1) + self.iadd.double().view(n, cin, 1, 1)
        if row.ops in ("in_act", "in_sft"):
            a = lrelu64(a, 0.2)
        if row.kind == "convt":
            y = F.conv_transpose2d(a, wt, b, stride=2)
        elif row.kind == "dgemm":                           # dx[ci] = sum over (a, b, co) of dy[(a, b), co] * W[ci][co][a][b]; x holds dy space-to-depth
            y = F.conv2d(a, wt.permute(0, 2, 3, 1).reshape(cout, cin, 1, 1))
        else:
            y = F.conv2d(a, wt, b, stride=row.stride, padding=1)
        if row.kind == "planar":
            op, sf = P_OPS[row.ops]
            ch, cw = CROP(row)
            y = y[..., :ch, :cw]
            if op == "add":
                y = y + (F.interpolate(self.res.double(), scale_factor=sf, mode="nearest") if sf > 1 else self.res.double())
            if op == "expclamp":
                assert int((y > CLAMP[1]).sum()) > 0 and int((y < CLAMP[0]).sum()) > 0 and int(((y > CLAMP[0]) & (y < CLAMP[1])).sum()) > 0
                y = torch.exp(torch.clamp(y, min=CLAMP[0], max=CLAMP[1]))
            return [y]
        if row.ops in ("mask_res", "mask"):
            y = y * torch.where(self.mask > 0, 1.0, 0.2).double()
        if row.ops in ("bias_res", "mask_res", "bridge"):
            y = y + self.res.double()
        if row.ops == "act":
            return [lrelu64(y, 0.25)]
        if row.ops == "dual":
            return [y, lrelu64(y, 0.25)]
        if row.ops == "sft":
            return [y, lrelu64(y * self.omul.double().view(n, cout, 1, 1) + self.oadd.double().view(n, cout, 1, 1), 0.25)]
        return [y]


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_instantiation_against_fp64_and_the_single_slab_tile(monkeypatch, row):
    setenv(monkeypatch, row.env)
    case = Case(row)
    refs = case.reference()
    planar = row.kind == "planar"
    # (a) + (b) under the row's knobs
    outs, keys, tiles = case.run()
    assert keys == [row.tile[:4]] and tiles == [("direct", row.tile)], (keys, tiles)
    assert len(outs) == len(refs)
    got = [(o.cpu() if planar else nchw(o)).double() for o in outs]
    assert all(tuple(g.shape) == tuple(r.shape) for g, r in zip(got, refs))
    errs = [float((g - r).abs().max()) for g, r in zip(got, refs)]
    bars = [5e-6 * float(r.max()) if row.ops == "expclamp" else TOL for r in refs]          # (tests/test_ops_gpu.py test_thin_output_epilogues)
    print(f"{row.id}: max error against fp64 {errs}, bar {bars}, largest reference element {[float(r.abs().max()) for r in refs]}")
    assert all(e <= b for e, b in zip(errs, bars)), (errs, bars)
    # (c) <KS, STRIDE, 1, 1>, four waves, on the same tensors: the same bits
    setenv(monkeypatch, row.single)
    singles, keys1, tiles1 = case.run()
    single = (row.ks, row.stride, 1, 1, 4)
    assert keys1 == [single[:4]] and tiles1 == [("direct", single)], (keys1, tiles1)
    for i, (o, s) in enumerate(zip(outs, singles)):
        assert torch.equal(o, s), (i, float((o - s).abs().max()))
