"""One table of the latency-class kernels of csrc/small.hip and the host launch branches in front of them: KNet's 9x9 stride-4 head with
its two gradients, the planar GAP with its finishing ops, the CALayer gate / scale / fused form, the SFT generators, the SFT backward
(atomic and ordered entry) and the NaN poisoner.  A row names a family, the C entries it runs, a shape, options and the branch it is
there for; each shape is the smallest that reaches its branch.  tests/test_small_coverage.py (CPU) works out from a row's shape which
host branches it takes and holds the table to the branch list and to the value sets it must span; tests/test_small_kernels_gpu.py runs
every row against the fp64 references below with NaN-filled outputs.

Below the table: the seeded inputs of a row (CPU fp32 tensors, `inputs`), the plain-torch fp64 reference of its operation (`reference`;
with drop=True the same with ONE term removed from every reduction the kernel performs, which the coverage test holds against the bar),
torch's own CPU fp32 evaluation for the rows whose sums are longer than anything the bars were set on (`fp32_error`), and the bars.

Bars (tests/test_ops_gpu.py, test_input_grad_gpu.py, test_sisr_train_gpu.py hold the same kernels to them against fp32): head forward and
dgrad 2e-5; gate / scale / fused / gap / sft_vec 1e-6; sft_apply 2e-6; sft_backward dx 1e-6, its sums and the head wgrad 2e-5 -- each
times max(1, max|ref|).  A row with long=True gets max(that, 4 * E32), E32 the largest error of torch's CPU fp32 evaluation of the same
operation on the same inputs: a different summation order of the same fp32 roundings, an order of magnitude under a dropped term.

No device is needed to import or to evaluate anything here."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from virnet_amd import _native

Row = namedtuple("Row", "id family entries shape opt why")
GAP_MEAN, GAP_EXPCLAMP, GAP_KINFO = _native.GAP_MEAN, _native.GAP_EXPCLAMP, _native.GAP_KINFO
FINISH = {GAP_MEAN: "mean", GAP_EXPCLAMP: "expclamp", GAP_KINFO: "kinfo"}
SLOPE = 0.2
CLAMP = (-1.0, 1.0)                                        # (lo, hi) of the GAP rows
KINK = 1e-3                                                # |x*mul+add| of the sft_backward rows stays at or above this (fp64)

BAR_HEAD, BAR_GATE, BAR_APPLY, BAR_DX, BAR_SUM = 2e-5, 1e-6, 2e-6, 1e-6, 2e-5


def _head(n, cin, h, w, cout, why, **opt):
    return Row(f"head-n{n}c{cin}h{h}w{w}-o{cout}", "head", ("virnet_conv_head_s4",), dict(n=n, cin=cin, h=h, w=w, cout=cout), opt, why)


def _wgrad(n, cin, h, w, cout, why, **opt):
    return Row(f"hwgrad-n{n}c{cin}h{h}w{w}-o{cout}", "head_wgrad", ("virnet_conv_head_s4_wgrad",), dict(n=n, cin=cin, h=h, w=w, cout=cout), opt, why)


def _dgrad(n, cin, h, w, cout, why):
    return Row(f"hdgrad-n{n}c{cin}h{h}w{w}-o{cout}", "head_dgrad", ("virnet_conv_head_s4_dgrad",), dict(n=n, cin=cin, h=h, w=w, cout=cout), {}, why)


def _gap(n, c, h, w, finish, why, **opt):
    return Row(f"gap-n{n}c{c}h{h}w{w}-{FINISH[finish]}", "gap", ("virnet_gap_nchw",), dict(n=n, c=c, h=h, w=w), dict(finish=finish, **opt), why)


def _ca(n, h, w, c, cr, why, **opt):
    return Row(f"ca-n{n}h{h}w{w}-c{c}r{cr}", "ca", ("virnet_ca_gate", "virnet_scale_add"), dict(n=n, h=h, w=w, c=c, cr=cr), opt, why)


def _fused(hw, c, cr, why, **opt):
    tag = "fallback" if opt.get("fallback") else "fused"
    return Row(f"{tag}-n3hw{hw}-c{c}r{cr}", "fused", ("virnet_ca_scale_add",), dict(n=3, h=1, w=hw, c=c, cr=cr), opt, why)


def _sftv(nf, e, why, **opt):
    return Row(f"sftvec-nf{nf}e{e}", "sft_vec", ("virnet_sft_vec",), dict(n=3, nf=nf, e=e), opt, why)


def _multi(layers, why):
    return Row(f"sftmulti-l{layers}", "sft_multi", ("virnet_sft_vec_multi", "virnet_sft_vec"), dict(n=3, layers=layers, e=4), {}, why)


def _apply(nf, e, n, h, w, step, chan0, why, **opt):
    return Row(f"sftapply-nf{nf}e{e}-n{n}h{h}w{w}-s{step}k{chan0}", "sft_apply", ("virnet_sft_apply",),
               dict(nf=nf, e=e, n=n, h=h, w=w, step=step, chan0=chan0), opt, why)


def _sftb(n, hw, c, res, why, **opt):
    return Row(f"sftb-n{n}hw{hw}c{c}-{'res' if res else 'nores'}" + ("-zero" if opt.get("zero") else ""), "sft_backward",
               ("virnet_sft_backward", "virnet_sft_backward_ordered"), dict(n=n, hw=hw, c=c), dict(res=res, **opt), why)


def _poison(n, why):
    return Row(f"poison-n{n}", "poison", ("virnet_poison_on_flag",), dict(n=n), {}, why)


ROWS = [
    # ---- conv_head_s4: 4 pixel slots x 64 channels per block, ppb pixels per block, grid.y = channel tile
    _head(1, 1, 1, 1, 64, "one output pixel: three idle pixel slots, K = 81 < 256 staging threads"),
    _head(1, 3, 3, 4, 64, "one output pixel of three channels; h % 4 = 3, w % 4 = 0"),
    _head(3, 3, 4, 5, 64, "six pixels: the second group has two live slots; a pixel group spans images"),
    _head(3, 3, 4, 5, 128, "... and the second channel tile (blockIdx.y = 1)"),
    _head(2, 3, 21, 30, 64, "the shape tests/test_ops_gpu.py::test_knet_pieces runs; w % 4 = 2"),
    _head(2, 3, 21, 30, 128, "... with the second channel tile"),
    _head(1, 4, 9, 7, 64, "four input channels, w % 4 = 3"),
    _head(5, 3, 5, 8, 64, "five images of 2 x 2 pixels: every group of four crosses an image"),
    _head(3, 2, 2, 2, 64, "three pixels (npix % 4 = 3), h % 4 = 2"),
    _head(2, 7, 6, 9, 128, "cin = 7: the largest LDS weight tile (156 492 of 163 840 bytes), both channel tiles"),
    _head(1, 1, 516, 516, 64, "16 641 pixels: ppb = 8, a block walks two pixel groups; bitwise against the 64 x 64 crop run (ppb = 4)", crop=64),
    _head(1, 8, 4, 4, 64, "cin = 8 does not fit the LDS weight tile: refused, nothing launched", refuse="LDS weight tile"),
    # ---- conv_head_s4_wgrad: block per (ci, ky, kx), rows split over four waves, two-pixel unroll, 64 channels per pass
    _wgrad(1, 1, 3, 4, 64, "ow = 1: only the unroll tail; n*oh = 1: three waves have no row"),
    _wgrad(3, 3, 4, 5, 96, "ow = 2: no tail; n*oh = 3; cout = 96: second pass with the co < cout guard"),
    _wgrad(1, 3, 8, 18, 128, "ow = 5: two unrolled pairs and the tail; n*oh = 2; cout = 128: two full passes"),
    _wgrad(2, 3, 21, 30, 64, "ow = 8, n*oh = 12: the shape of the red-zone run"),
    _wgrad(5, 1, 5, 8, 64, "ow = 2, n*oh = 10 (% 4 = 2), one input channel"),
    _wgrad(1, 3, 592, 592, 64, "21 904 terms per element: the long sum", long=True),
    # ---- conv_head_s4_dgrad: thread per input element, grid capped at 4096 blocks
    _dgrad(1, 3, 64, 64, 64, "tests/test_input_grad_gpu.py's four shapes"),
    _dgrad(3, 3, 57, 86, 64, "..."),
    _dgrad(1, 3, 9, 7, 64, "..."),
    _dgrad(3, 3, 13, 13, 64, "..."),
    _dgrad(1, 3, 9, 7, 4, "cout = 4: one channel quad"),
    _dgrad(3, 3, 13, 13, 96, "cout = 96: 24 quads, six passes of the unroll-by-4 loop"),
    _dgrad(1, 3, 592, 592, 64, "1 051 392 elements > 4096 x 256: the grid-stride pass"),
    # ---- gap_nchw: block per plane, 256 threads
    _gap(3, 3, 1, 1, GAP_MEAN, "hw = 1: 255 idle threads"),
    _gap(3, 3, 1, 1, GAP_KINFO, "hw = 1, exp(clamp) on two channels (below / inside / above) and tanh on the third"),
    _gap(2, 3, 7, 9, GAP_EXPCLAMP, "hw = 63: less than a wave"),
    _gap(3, 1, 15, 17, GAP_KINFO, "hw = 255; c = 1: the only channel is the tanh one"),
    _gap(2, 3, 16, 16, GAP_MEAN, "hw = 256: one element per thread"),
    _gap(2, 3, 16, 16, GAP_EXPCLAMP, "hw = 256"),
    _gap(3, 3, 1, 257, GAP_KINFO, "hw = 257: thread 0 takes a second element"),
    _gap(1, 3, 481, 321, GAP_MEAN, "154 401 elements per plane: the long sum", long=True),
    # ---- ca_gate (256 / c pixel phases x c channels) + scale_add (grid capped at 8192 blocks)
    _ca(2, 1, 1, 4, 1, "hw = 1 < 64 pixel phases; cr = 1"),
    _ca(2, 1, 3, 64, 4, "hw = 3 < 4 pixel phases"),
    _ca(2, 1, 3, 4, 64, "cr = 64 > c: the full f1 array"),
    _ca(2, 15, 17, 64, 4, "hw = 255, KernelNet's widths"),
    _ca(1, 257, 1, 256, 64, "c = 256: one pixel phase, hw = 257; cr = 64"),
    _ca(1, 3, 85, 256, 1, "c = 256, hw = 255, cr = 1"),
    _ca(3, 1, 257, 4, 4, "c = 4: 64 pixel phases, hw = 257 = 4 x 64 + 1"),
    _ca(1, 1, 1, 96, 4, "c = 96 does not divide 256: virnet_ca_gate refuses", refuse="must divide 256"),
    Row("scaleadd-n1h363w363-c64", "scale_add", ("virnet_scale_add",), dict(n=1, h=363, w=363, c=64), {},
        "2 108 304 float4 items > 8192 x 256: the grid-stride pass"),
    # ---- ca_scale_add: an image in one workgroup's registers, V float4 items per thread; both sides of each V limit
    _fused(1, 4, 1, "one item: V = 4 with 1023 idle threads"),
    _fused(4096, 4, 1, "4096 items: V = 4 full"),
    _fused(4097, 4, 1, "4097 items: V = 8, first side"),
    _fused(8192, 4, 4, "8192 items: V = 8 full"),
    _fused(8193, 4, 4, "8193 items: V = 16 (skip loaded late)"),
    _fused(16384, 4, 4, "16 384 items: V = 16 full, the limit"),
    _fused(256, 64, 4, "KernelNet's 16 x 16 x 64 map: V = 4 full"),
    _fused(257, 64, 4, "V = 8"),
    _fused(512, 64, 4, "V = 8 full"),
    _fused(513, 64, 4, "V = 16"),
    _fused(1024, 64, 4, "V = 16 full"),
    _fused(64, 256, 64, "c = 256, cr = 64: every LDS array full, 64 channel quads"),
    _fused(16385, 4, 1, "16 385 items: the direct ABI call is refused", refuse="does not fit one workgroup"),
    _fused(16385, 4, 1, "16 385 items through ops.ca_scale_add: the gate + scale launches", fallback=True),
    # ---- sft_vec: AttLayer on a per-image vector, block per image
    _sftv(96, 4, "the denoiser's first level"),
    _sftv(288, 4, "its deepest level: the second pass of the c += 256 loop (32 channels)"),
    _sftv(512, 16, "e = 16, nf1 = 64, nf2 = 128: every LDS array exactly full, two full channel passes"),
    _sftv(64, 1, "one conditioning channel"),
    _sftv(520, 4, "nf1 = 65 does not fit: check_sft refuses", refuse="unsupported widths"),
    # ---- sft_vec_multi: 16 layers per launch
    _multi(1, "one layer, one launch"),
    _multi(16, "a full launch"),
    _multi(17, "two launches, the second of one layer"),
    _multi(33, "three launches"),
    # ---- sft_apply: 16 pixels per block, AttLayer per pixel from a 16-channel record sampled every `step` pixels
    _apply(96, 4, 1, 3, 5, 1, 0, "15 pixels: one idle pixel slot"),
    _apply(288, 4, 2, 2, 4, 2, 3, "16 pixels over two images, step 2, channels 3..6; second channel pass"),
    _apply(512, 16, 1, 1, 17, 4, 0, "17 pixels: a second block of one; step 4; full LDS arrays, the whole record"),
    _apply(64, 1, 3, 5, 1, 2, 3, "15 pixels over three images, one conditioning channel"),
    _apply(104, 13, 1, 17, 1, 1, 3, "e = 13 at chan0 = 3: the last record channel is read"),
    _apply(104, 13, 1, 4, 4, 1, 4, "chan0 + e = 17: outside the record, refused", refuse="outside the 16-channel record"),
    # ---- sft_backward: blocks of 1024 pixels x n images, 256 / c4 pixel lanes
    _sftb(1, 1, 4, False, "one pixel, c4 = 1: 255 idle pixel lanes"),
    _sftb(3, 1, 1024, False, "one pixel, c4 = 256: one pixel lane"),
    _sftb(3, 1023, 8, True, "one short chunk"),
    _sftb(1, 1024, 96, True, "exactly one chunk; c4 = 24 does not divide 256: sixteen idle threads"),
    _sftb(3, 1025, 96, False, "two chunks, the second of one pixel"),
    _sftb(1, 2049, 1024, True, "three chunks, one pixel lane: 1024 terms per block and thread", long=True),
    _sftb(3, 2049, 4, False, "three chunks, 256 pixel lanes", long=True),
    _sftb(1, 33, 8, True, "u == 0 exactly at chosen positions: the derivative there is the slope branch (torch's convention)", zero=True),
    # ---- poison_on_flag: grid capped at 1024 blocks
    _poison(1, "one element"),
    _poison(255, "less than a block"),
    _poison(256 * 1024 + 1, "one element more than the capped grid covers in one pass"),
]
BY_ID = {r.id: r for r in ROWS}


def rows(family, refused=False):
    return [r for r in ROWS if r.family == family and bool(r.opt.get("refuse")) == refused]


def out_hw(h, w):
    """output size of the 9x9 stride-4 pad-4 head"""
    return (h - 1) // 4 + 1, (w - 1) // 4 + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = np.random.Generator(np.random.Philox(key=[seed, int(np.prod(shape)) & 0xFFFFFFFF]))
    return torch.from_numpy((g.random(size=shape, dtype=np.float32) * (hi - lo) + lo).astype(np.float32))


def make_att(nf, e, seed):
    """an AttLayer with torch's default initialisation under a fixed seed (what tests/test_ops_gpu.py::test_sft_generators uses)"""
    from virnet_amd.networks.AttResUNet import AttLayer
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return AttLayer(nf, e)


MULTI_NF = (96, 288, 160, 64)                              # widths of sft_vec_multi's layers, in turn


def _ca_inputs(s, seed):
    """hcv = 4 * U(-1, 1) + a per-channel offset (so the means are O(1) at every hw and one term weighs 4 / hw), weights of gain ~ 1"""
    n, hw, c, cr = s["n"], s["h"] * s["w"], s["c"], s["cr"]
    hcv = 4.0 * rnd(n, hw, c, seed=seed) + rnd(1, 1, c, seed=seed + 1)
    g1, g2 = min(1.0, 2.0 / c ** 0.5), min(1.0, 2.0 / cr ** 0.5)
    return dict(hcv=hcv, skip=rnd(n, hw, c, seed=seed + 2), w1=rnd(cr, c, seed=seed + 3) * g1, b1=rnd(cr, seed=seed + 4) * 0.1,
                w2=rnd(c, cr, seed=seed + 5) * g2, b2=rnd(c, seed=seed + 6) * 0.1)


def _sftb_inputs(row):
    n, hw, c = row.shape["n"], row.shape["hw"], row.shape["c"]
    x, da = rnd(n, hw, c, seed=70, lo=-0.5, hi=0.5), rnd(n, hw, c, seed=71, lo=-0.5, hi=0.5)
    mul, add = rnd(n, c, seed=72, lo=0.3, hi=1.3), rnd(n, c, seed=73, lo=-0.5, hi=0.5)
    zero = None
    if row.opt.get("zero"):                                # channels 1 and 6 of image 0 get add = 0, and x = 0 at every third pixel
        add[0, 1] = add[0, 6] = 0.0
        zero = torch.zeros(n, hw, c, dtype=torch.bool)
        zero[0, ::3, 1] = zero[0, 1::3, 6] = True
    # push x away from the kink: where |x*mul+add| < KINK in fp64, move x by 4*KINK/mul in the direction u already has
    for _ in range(2):
        u = x.double() * mul.double()[:, None, :] + add.double()[:, None, :]
        near = u.abs() < KINK
        x = torch.where(near, x + (torch.where(u < 0, -4.0, 4.0) * KINK / mul.double()[:, None, :]).float(), x)
    if zero is not None:
        x = torch.where(zero, torch.zeros_like(x), x)
    out = dict(x=x, da=da, mul=mul, add=add, res=rnd(n, hw, c, seed=74, lo=-0.5, hi=0.5) if row.opt["res"] else None)
    if zero is not None:
        out["zero"] = zero
    return out


def inputs(row):
    """CPU fp32 tensors of a row (None for a refusal row that needs no values)"""
    s, f = row.shape, row.family
    if f in ("head", "head_wgrad", "head_dgrad"):
        n, cin, h, w, cout = s["n"], s["cin"], s["h"], s["w"], s["cout"]
        oh, ow = out_hw(h, w)
        return dict(x=rnd(n, cin, h, w, seed=22, lo=0.0, hi=1.0), wt=rnd(cout, cin, 9, 9, seed=21) * 0.06, dy=rnd(n, cout, oh, ow, seed=23))
    if f == "gap":
        n, c, h, w = s["n"], s["c"], s["h"], s["w"]
        # plane (img, ch) sits around -2.5, 0.2 or 2.5 with amplitude 0.5: its mean lands below lo, inside the clamp or above hi
        off = torch.tensor([[(-2.5, 0.2, 2.5)[(i + ch) % 3] for ch in range(c)] for i in range(n)])
        return dict(x=rnd(n, c, h, w, seed=29, lo=-0.5, hi=0.5) + off[:, :, None, None])
    if f in ("ca", "fused"):
        return _ca_inputs(s, 50)
    if f == "scale_add":
        n, hw, c = s["n"], s["h"] * s["w"], s["c"]
        return dict(hcv=rnd(n, hw, c, seed=60), skip=rnd(n, hw, c, seed=61), gate=rnd(n, c, seed=62, lo=0.0, hi=1.0))
    if f == "sft_vec":
        return dict(att=make_att(s["nf"], s["e"], 31), vec=rnd(s["n"], s["e"], seed=31, lo=0.0, hi=1.5))
    if f == "sft_multi":
        return dict(atts=[make_att(MULTI_NF[l % 4], s["e"], 34 + l) for l in range(s["layers"])], vec=rnd(s["n"], s["e"], seed=35, lo=0.0, hi=1.5))
    if f == "sft_apply":
        n, h, w, step = s["n"], s["h"], s["w"], s["step"]
        return dict(att=make_att(s["nf"], s["e"], 32), rec=rnd(n, h * step, w * step, 16, seed=32, lo=0.0, hi=1.0), raw=rnd(n, h, w, s["nf"], seed=33))
    if f == "sft_backward":
        return _sftb_inputs(row)
    if f == "poison":
        return dict(y=rnd(s["n"], seed=80))
    raise KeyError(f)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def lrelu64(t, slope=SLOPE):
    return torch.where(t > 0, t, t * slope)


def att64(att, e):
    """AttLayer in fp64 on channels-last conditioning e [..., e]: (mul, add), each [..., nf]"""
    def lin(conv, t):
        return t @ conv.weight.detach().double().flatten(1).T + conv.bias.detach().double()
    f2 = lrelu64(lin(att.conv2, lrelu64(lin(att.conv1, e.double()))))
    return torch.sigmoid(lin(att.mul_conv, f2)), lin(att.add_conv, f2)


def _mean_drop(t, dim):
    """(sum - the term of largest magnitude) / count along dim: the mean with one term missing"""
    big = t.gather(dim, t.abs().argmax(dim, keepdim=True)).squeeze(dim)
    return (t.sum(dim) - big) / t.shape[dim]


def ca64(inp, drop=False):
    """CALayer + skip in fp64 on [n, hw, c]: (gate [n, c], hcv * gate + skip)"""
    h = inp["hcv"].double()
    mean = _mean_drop(h, 1) if drop else h.mean(1)
    f1 = lrelu64(mean @ inp["w1"].double().T + inp["b1"].double())
    gate = torch.sigmoid(f1 @ inp["w2"].double().T + inp["b2"].double())
    return gate, h * gate[:, None, :] + inp["skip"].double()


def gap_finish(mean, finish, c):
    lo, hi = CLAMP
    if finish == GAP_MEAN:
        return mean
    ex = torch.exp(mean.clamp(lo, hi))
    if finish == GAP_EXPCLAMP:
        return ex
    return torch.cat([ex[:, :c - 1], torch.tanh(mean[:, c - 1:])], 1)


def head_wgrad_autograd(x, dy, cout, dtype):
    wt = torch.zeros(cout, x.shape[1], 9, 9, dtype=dtype, requires_grad=True)
    F.conv2d(x.to(dtype), wt, None, stride=4, padding=4).backward(dy.to(dtype))
    return wt.grad


def sftb_autograd(inp, dtype):
    """(dx without res, dmul, dadd) by autograd in `dtype`"""
    x, mul, add = (inp[k].detach().clone().to(dtype).requires_grad_(True) for k in ("x", "mul", "add"))
    F.leaky_relu(x * mul[:, None, :] + add[:, None, :], SLOPE).backward(inp["da"].to(dtype))
    return x.grad, mul.grad, add.grad


def reference(row, inp, drop=False):
    """dict of the row's outputs in fp64 (layouts as the kernels store them).  drop: one term is missing from every sum the kernel reduces."""
    s, f = row.shape, row.family
    if f == "head":
        return dict(out=F.conv2d(inp["x"].double(), inp["wt"].double(), None, stride=4, padding=4).permute(0, 2, 3, 1).contiguous())
    if f == "head_wgrad":
        dw = head_wgrad_autograd(inp["x"], inp["dy"], s["cout"], torch.float64)
        if drop:                                           # the products of output pixel (0, oh/2, ow/2) leave every element whose tap is inside the image
            oh, ow = out_hw(s["h"], s["w"])
            oy, ox = oh // 2, ow // 2
            xp = F.pad(inp["x"].double(), (4, 4, 4, 4))
            dw = dw - inp["dy"].double()[0, :, oy, ox][:, None, None, None] * xp[0, :, 4 * oy:4 * oy + 9, 4 * ox:4 * ox + 9][None]
        return dict(dw=dw)
    if f == "head_dgrad":
        x0 = torch.zeros(s["n"], s["cin"], s["h"], s["w"], dtype=torch.float64, requires_grad=True)
        F.conv2d(x0, inp["wt"].double(), None, stride=4, padding=4).backward(inp["dy"].double())
        return dict(dx=x0.grad)
    if f == "gap":
        planes = inp["x"].double().flatten(2)
        return dict(out=gap_finish(_mean_drop(planes, 2) if drop else planes.mean(2), row.opt["finish"], s["c"]))
    if f == "ca":
        gate, out = ca64(inp, drop)
        return dict(gate=gate, out=out)
    if f == "fused":
        return dict(out=ca64(inp, drop)[1])
    if f == "scale_add":
        return dict(out=inp["hcv"].double() * inp["gate"].double()[:, None, :] + inp["skip"].double())
    if f == "sft_vec":
        mul, add = att64(inp["att"], inp["vec"])
        return dict(mul=mul, add=add)
    if f == "sft_multi":
        return dict(layers=[att64(att, inp["vec"]) for att in inp["atts"]])
    if f == "sft_apply":
        step, k0 = s["step"], s["chan0"]
        mul, add = att64(inp["att"], inp["rec"][:, ::step, ::step, k0:k0 + s["e"]])
        return dict(act=lrelu64(inp["raw"].double() * mul + add))
    if f == "sft_backward":
        x, da, mul, add = (inp[k].double() for k in ("x", "da", "mul", "add"))
        u = x * mul[:, None, :] + add[:, None, :]
        du = torch.where(u > 0, da, da * SLOPE)            # u == 0 takes the slope, as torch.nn.functional.leaky_relu's backward does
        dx = du * mul[:, None, :] + (inp["res"].double() if inp["res"] is not None else 0.0)
        tm, ta = du * x, du
        if drop:                                           # pixel hw/2 of every image is missing from both sums
            keep = torch.ones(s["hw"], dtype=torch.float64)
            keep[s["hw"] // 2] = 0.0
            tm, ta = tm * keep[None, :, None], ta * keep[None, :, None]
        return dict(dx=dx, dmul=tm.sum(1), dadd=ta.sum(1))
    if f == "poison":                                      # (held to bit patterns, not to a reference)
        return {}
    raise KeyError(f)


def fp32_error(row, inp, ref):
    """E32 of a long row: {output: largest error of torch's CPU fp32 evaluation of the same operation against `ref`}"""
    assert row.opt.get("long"), row.id
    f = row.family
    if f == "head_wgrad":
        got = dict(dw=head_wgrad_autograd(inp["x"], inp["dy"], row.shape["cout"], torch.float32))
    elif f == "gap":
        got = dict(out=gap_finish(inp["x"].mean((2, 3)), row.opt["finish"], row.shape["c"]))
    elif f == "sft_backward":
        _, dmul, dadd = sftb_autograd(inp, torch.float32)
        got = dict(dmul=dmul, dadd=dadd)
    else:
        raise KeyError(f)
    return {k: float((v.double() - ref[k]).abs().max()) for k, v in got.items()}


EXISTING_BAR = {("head", "out"): BAR_HEAD, ("head_dgrad", "dx"): BAR_HEAD, ("head_wgrad", "dw"): BAR_SUM, ("gap", "out"): BAR_GATE,
                ("ca", "gate"): BAR_GATE, ("ca", "out"): BAR_GATE, ("fused", "out"): BAR_GATE, ("scale_add", "out"): BAR_GATE,
                ("sft_vec", "mul"): BAR_GATE, ("sft_vec", "add"): BAR_GATE, ("sft_multi", "mul"): BAR_GATE, ("sft_multi", "add"): BAR_GATE,
                ("sft_apply", "act"): BAR_APPLY, ("sft_backward", "dx"): BAR_DX, ("sft_backward", "dmul"): BAR_SUM, ("sft_backward", "dadd"): BAR_SUM}
REDUCED = {"head_wgrad": ("dw",), "gap": ("out",), "ca": ("gate", "out"), "fused": ("out",), "sft_backward": ("dmul", "dadd")}   # outputs behind a sum over pixels


def bar(row, key, ref, e32=None):
    """absolute bar of output `key`: the existing bar x max(1, max|ref|); a long row's reduced outputs get max(that, 4 x E32)"""
    b = EXISTING_BAR[(row.family, key)] * max(1.0, float(ref.abs().max()))
    if row.opt.get("long") and key in REDUCED.get(row.family, ()):
        b = max(b, 4.0 * e32[key])
    return b


class Case:
    """inputs, fp64 reference, E32 (long rows) and bars of a row"""

    def __init__(self, row):
        self.row, self.inp = row, inputs(row)
        self.ref = reference(row, self.inp)
        self.e32 = fp32_error(row, self.inp, self.ref) if row.opt.get("long") else None

    def bar(self, key):
        return bar(self.row, key, self.ref[key], self.e32)


@functools.lru_cache(maxsize=None)
def case(rid):
    """the Case of a row, built once per process and left unchanged"""
    return Case(BY_ID[rid])
