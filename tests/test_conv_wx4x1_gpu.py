"""GPU tests of the one-product fp16 Winograd form (csrc/conv_f16_wx4x1.hip, VIRNET_CONV_FORM=wx4x1): reduced precision, inference only.

What "right" means for a reduced-precision kernel.  Three errors against an fp64 convolution of the same fp32 tensors:
  e_k  the kernel's        e_m  the CPU emulation's (tests/wx4x1_ref.py: the arithmetic the header states)
  e_b  an fp64 convolution of bf16-rounded operands (the arithmetic of the form this one is meant to beat)
Bars:  A. max |kernel - emulation| <= 0.5 e_m -- the kernel computes the stated arithmetic.  Two orderings of the emulation differ by up to
          0.12 e_m at these shapes on the CPU (an fp32-ulp difference in V flips an fp16 rounding now and then): a fourfold margin.
       B. 0.5 e_m <= e_k <= 1.5 e_m -- as inaccurate as stated, not more, and (lower bound) not the three-product path.
       C. e_k < e_b -- better than bf16; tests/test_wx4x1_host.py holds e_m <= 0.7 e_b for the same inputs on the CPU.
End to end the bars come from the numerics gate (tools/numerics_gate.py), computed here on the CPU for the tested size."""
import importlib.util
import json
import os

import pytest
import torch
import torch.nn.functional as F

import wx4x1_ref
from virnet_amd import engine, ops
from virnet_amd.networks import VIRAttResUNet, VIRAttResUNetSR
from virnet_amd.utils.synth import synth_images, synth_state_dict
from test_ops_gpu import make_conv, nchw, nhwc, rnd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM = "wx4x1"


@pytest.fixture(autouse=True)
def _form(monkeypatch):
    for k in ("VIRNET_WINOGRAD", "VIRNET_WX4_ROWS", "VIRNET_WX4_NREP", "VIRNET_RANGE_GUARD", "VIRNET_DETERMINISTIC"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VIRNET_CONV_FORM", FORM)
    monkeypatch.setenv("VIRNET_WX4_MIN_TILES", "0")      # every shape through the kernel under test, also the ones the shape rule
    monkeypatch.setenv("VIRNET_WX4_MIN_COUT", "0")       # would hand to conv_f16 (small images, 32 / 64 channels)
    monkeypatch.setenv("VIRNET_WX4_MIN_FILL", "0")
    monkeypatch.setenv("VIRNET_WX4_MIN_WGS", "0")


class ops_timer:
    def __enter__(self):
        self.t = ops.LaunchTimer()
        ops.set_launch_timer(self.t)
        return self.t

    def __exit__(self, *exc):
        ops.set_launch_timer(None)
        return False


def bars(got: torch.Tensor, ref: torch.Tensor, emu: torch.Tensor, e_m: float, e_b: float, what=""):
    e_k = float((got.double() - ref).abs().max())
    d = float((got.double() - emu.double()).abs().max())
    print(f"{what}: e_k {e_k:.3e}  e_m {e_m:.3e}  e_b {e_b:.3e}  |kernel - emulation| {d:.3e} = {d / e_m:.3f} e_m")
    assert d <= 0.5 * e_m, ("A", what, d, e_m)
    assert 0.5 * e_m <= e_k <= 1.5 * e_m, ("B", what, e_k, e_m)
    assert e_k < e_b, ("C", what, e_k, e_b)


# (the shapes leave CUs empty, so the plan gives every launch ONE slab per workgroup; VIRNET_WX4_NREP pins the grouping for the three extra
#  cases: 288 = 3 x 3 slabs, 160 = 3 + 2, 64 = 2)
CASES = [s + (None,) for s in wx4x1_ref.SHAPES] + [(288, 16, 64, 1, "3"), (160, 18, 40, 1, "3"), (64, 9, 33, 2, "2")]


@pytest.mark.parametrize("c,h,w,n,nrep", CASES)
def test_wx4x1_layer_against_emulation_fp64_and_bf16(monkeypatch, c, h, w, n, nrep):
    """Odd sizes (partial tiles in both directions, halo rows beyond the image), 1 to 9 slabs, pre-activation, residual + dual store."""
    if nrep is not None:
        monkeypatch.setenv("VIRNET_WX4_NREP", nrep)
    cp = make_conv(c, c, seed=80)
    x, res = rnd(n, c, h, w, seed=81), rnd(n, c, h, w, seed=82)
    ref, emu, e_m, e_b = wx4x1_ref.three_errors(F.leaky_relu(x, 0.2), cp.weight.detach(), cp.bias.detach(), lambda y: y + res.to(y.dtype))
    cp.cuda()
    pw = cp.packed()
    assert pw.wx4 is not None
    with ops_timer() as t:
        raw, act = ops.conv_mfma(nhwc(x), pw, in_slope=0.2, res=nhwc(res), want_raw=True, want_act=True, slope=0.25)
        raw2, _ = ops.conv_mfma(nhwc(x), pw, in_slope=0.2, res=nhwc(res), want_raw=True, want_act=True, slope=0.25)
    assert [k[0] for k in t.summary()] == [FORM]
    assert torch.equal(raw, raw2)                              # two runs of one launch: bit for bit
    assert torch.equal(act, torch.maximum(raw, raw * 0.25))
    bars(nchw(raw), ref, emu, e_m, e_b, f"c{c} {n}x{h}x{w}")


@pytest.mark.parametrize("epi", ["plain", "act", "res", "mask", "mask_res", "sft_out"])
def test_wx4x1_epilogue_and_preactivation_forms(epi):
    """One instantiation per epilogue form (EPI 0..4) and pre-activation level (PRE 0..2) at 96 channels, 2 x 21 x 45, same three bars."""
    c, n, h, w = 96, 2, 21, 45
    cp = make_conv(c, c, seed=83)
    x, res, saved = rnd(n, c, h, w, seed=84), rnd(n, c, h, w, seed=85), rnd(n, c, h, w, seed=86)
    wt, b = cp.weight.detach(), cp.bias.detach()
    cp.cuda()
    pw = cp.packed()
    m = torch.where(saved > 0, 1.0, 0.2)
    xa, post, kw, out = x, (lambda y: y), dict(want_raw=True), 0
    if epi == "act":
        post, kw, out = (lambda y: F.leaky_relu(y, 0.2)), dict(want_raw=False, want_act=True, slope=0.2), 1
    elif epi == "res":
        xa, post, kw = F.leaky_relu(x, 0.2), (lambda y: y + res.to(y.dtype)), dict(in_slope=0.2, res=nhwc(res), want_raw=True)
    elif epi == "mask":
        post, kw = (lambda y: y * m.to(y.dtype)), dict(mask=nhwc(saved), mask_slope=0.2, want_raw=True)
    elif epi == "mask_res":
        post, kw = (lambda y: y * m.to(y.dtype) + res.to(y.dtype)), dict(mask=nhwc(saved), mask_slope=0.2, res=nhwc(res), want_raw=True)
    elif epi == "sft_out":
        imul, iadd = rnd(n, c, seed=87, lo=0.3, hi=1.0), rnd(n, c, seed=88)
        omul, oadd = rnd(n, c, seed=89, lo=0.3, hi=1.0), rnd(n, c, seed=90)
        xa = F.leaky_relu(x * imul.view(n, c, 1, 1) + iadd.view(n, c, 1, 1), 0.2)
        post = lambda y: y + res.to(y.dtype)      # noqa: E731
        kw = dict(in_slope=0.2, in_mul=imul.cuda(), in_add=iadd.cuda(), res=nhwc(res), mul=omul.cuda(), add=oadd.cuda(), want_raw=True, want_act=True, slope=0.2)
    ref, emu, e_m, e_b = wx4x1_ref.three_errors(xa, wt, b, post)
    with ops_timer() as t:
        outs = ops.conv_mfma(nhwc(x), pw, **kw)
    assert [k[0] for k in t.summary()] == [FORM]
    bars(nchw(outs[out]), ref, emu, e_m, e_b, epi)
    if epi == "sft_out":                                        # the second store: lrelu(raw * mul + add) of the SAME raw values, in fp32
        want = F.leaky_relu(nchw(outs[0]) * omul.view(n, c, 1, 1) + oadd.view(n, c, 1, 1), 0.2)
        assert float((nchw(outs[1]) - want).abs().max()) <= 4e-6 * float(want.abs().max())


def test_wx4x1_range_flag_trips_like_the_split_kernels():
    """The transformed magnitude is what must fit fp16: |x| = 5e3 passes, 3e4 (x 5 in B^T) trips the sticky flag and the result is not finite."""
    c, n, h, w = 96, 1, 16, 32
    cp = make_conv(c, c, seed=12).cuda()
    dev = torch.device("cuda", torch.cuda.current_device())
    flag = ops.range_flag(dev)
    assert flag is not None
    flag.zero_()
    x = rnd(n, c, h, w, seed=13)
    for amp, expect in ((5.0e3, False), (3.0e4, True)):
        xs = x.clone()
        xs[0, 5, 7, 9] = amp
        raw, _ = ops.conv_mfma(nhwc(xs), cp.packed(), want_raw=True)
        assert ops.range_overflowed(dev) is expect, amp
        assert bool(torch.isfinite(raw).all()) is (not expect), amp
    assert not ops.range_overflowed(dev)


def _net(kind="syn", seed=1234):
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        cfg = dict(json.load(f)["configs"][kind])
    sisr = cfg.pop("kind") == "sisr"
    net = (VIRAttResUNetSR if sisr else VIRAttResUNet)(**cfg)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=seed), strict=True)
    return net.cuda().eval()


def test_wx4x1_guard_reruns_the_forward_in_fp32(monkeypatch):
    """An image whose activations leave fp16's range inside the network: one re-run, and the result is the fp32 form's bit for bit."""
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")
    net = _net()
    x = synth_images(1, 3, 64, 64).cuda()
    x[0, :, 20:24, 20:24] = 3.0e4              # (the head conv amplifies this beyond 65504 inside RNet)
    with torch.no_grad():
        with ops.forward_scope(form=engine.FP32_FORM):
            ref = [t.clone() for t in engine._denoise_forward(net, x)]
        engine.guard_stats(reset=True)
        with pytest.warns(RuntimeWarning, match="fp16's range"):
            mu, sigma = net(x)
        assert engine.guard_stats() == {"forwards": 1, "reruns": 1}
        assert bool(torch.isfinite(mu).all()) and torch.equal(mu, ref[0]) and torch.equal(sigma, ref[1])


def _gate():
    spec = importlib.util.spec_from_file_location("numerics_gate", os.path.join(ROOT, "tools", "numerics_gate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wx4x1_denoise_syn_end_to_end_within_the_gate(monkeypatch):
    """Whole denoise-syn network, synthetic weights, N = 2 at 96^2, against fp64: within 2x the gate's wx4x1 row (the product routes a few
    launches differently from the gate's eligibility rule and sums in another order) and below the gate's bf16x1 row -- both rows computed
    here on the CPU for this very input."""
    monkeypatch.delenv("VIRNET_WX4_MIN_TILES"); monkeypatch.delenv("VIRNET_WX4_MIN_COUT"); monkeypatch.delenv("VIRNET_WX4_MIN_FILL")
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")
    rows, mu64, sg64, x = _gate().gate(96, 2, ["wx4x1", "bf16x1"])
    g1, gb = rows
    net = _net()
    with torch.no_grad(), ops_timer() as t:
        mu, sigma = net(x.cuda())
    names = [k[0] for k in t.summary()]
    assert FORM in names and "wx4" not in names, names
    e_mu = float((mu.cpu().double() - mu64).abs().max())
    e_sg = float(((sigma.cpu().double() - sg64).abs() / sg64.abs().clamp_min(1e-30)).max())
    print(f"mu max-abs {e_mu:.3e} (gate wx4x1 {g1['mu_max_abs']:.3e}, bf16x1 {gb['mu_max_abs']:.3e});  sigma max-rel {e_sg:.3e} "
          f"(gate {g1['sigma_max_rel']:.3e}, {gb['sigma_max_rel']:.3e})")
    assert e_mu <= 2 * g1["mu_max_abs"] and e_mu < gb["mu_max_abs"]
    assert e_sg <= 2 * g1["sigma_max_rel"] and e_sg < gb["sigma_max_rel"]


@pytest.mark.parametrize("kind", ["real", "sisr"])
def test_wx4x1_is_closer_to_the_default_form_than_bf16(monkeypatch, kind):
    """denoise-real (four levels, sigma_chn = 3) at 64^2 and SISR x2 from 32^2: the distance of mu (SISR: and of kinfo) from the default
    form's result is smaller under wx4x1 than under bf16, all three measured on the same input.
    SISR: KernelNet's body runs conv by conv here (VIRNET_KNET_PERSISTENT=0).  Its one-launch form (csrc/knet_body.hip) is the same
    kernel under every f16-family form, so kinfo would be bit-identical under all three and the comparison 0 < 0.  Conv by conv the bf16
    form reaches KernelNet's 64-channel convs; the Winograd forms do not (an 8 x 8 map fills an eighth of a tile: wx4_shape_ok sends it to
    f16x3 under wx4 and wx4x1 alike), so kinfo under wx4x1 IS the default form's and the distance is exactly 0."""
    if kind == "sisr":
        monkeypatch.setenv("VIRNET_KNET_PERSISTENT", "0")
    monkeypatch.delenv("VIRNET_WX4_MIN_TILES"); monkeypatch.delenv("VIRNET_WX4_MIN_COUT"); monkeypatch.delenv("VIRNET_WX4_MIN_FILL")
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")
    net = _net(kind)
    x = synth_images(2, 3, 64, 64).cuda() if kind == "real" else synth_images(2, 3, 32, 32).cuda()
    outs = {}
    with torch.no_grad():
        for form in ("wx4", FORM, "bf16"):
            monkeypatch.setenv("VIRNET_CONV_FORM", form)
            with ops_timer() as t:
                o = net(x) if kind == "real" else net(x, 2)
            outs[form] = [v.clone() for v in o]
            assert form in [k[0] for k in t.summary()], (form, list(t.summary()))
    for i in ((0,) if kind == "real" else (0, 1)):               # mu; SISR: kinfo as well
        d1 = float((outs[FORM][i] - outs["wx4"][i]).abs().max())
        db = float((outs["bf16"][i] - outs["wx4"][i]).abs().max())
        print(f"{kind} output {i}: |wx4x1 - default| {d1:.3e}   |bf16 - default| {db:.3e}")
        assert d1 < db, (kind, i, d1, db)
        assert d1 > 0.0 or i == 1, (kind, i, d1)                  # (mu: the form is really in the forward)


def test_wx4x1_eager_and_graph_replay_are_bitwise_equal():
    """net(x) four times: eager, eager, then the captured graph's replays -- one result."""
    net = _net()
    x = synth_images(2, 3, 48, 64).cuda()
    with torch.no_grad():
        outs = [[t.clone() for t in net(x)] for _ in range(4)]
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


def test_wx4x1_is_inference_only():
    """A forward recorded for autograd and the frozen network's image gradient raise, naming the form."""
    net = _net()
    x = synth_images(1, 3, 32, 32).cuda()
    with pytest.raises(RuntimeError, match="VIRNET_CONV_FORM=wx4x1 is an inference-only form"):
        net(x)                                                    # (grad mode, trainable parameters)
    net.requires_grad_(False)
    with pytest.raises(RuntimeError, match="VIRNET_CONV_FORM=wx4x1 is an inference-only form"):
        net(x.clone().requires_grad_(True))
    cp = make_conv(96, 96).cuda()
    with pytest.raises(RuntimeError, match="inference-only"):
        cp.packed_dgrad()
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.conv_mfma(torch.zeros(1, 16, 32, 96, device="cuda"), cp.packed(), emit=dict(act=None, colsum=None))
    with torch.no_grad():
        net(x)


@pytest.mark.parametrize("c,n,h,w,epi", [(96, 1, 17, 70, "plain"), (32, 1, 3, 2, "res"), (224, 1, 33, 31, "sft"), (64, 2, 9, 33, "mask"),
                                         (160, 1, 18, 40, "dual"), (192, 2, 6, 31, "preact")])
def test_wx4x1_red_zone(c, n, h, w, epi):
    """The new kernel between NaN-patterned guard zones (tests/redzone.py) at the partial-tile shapes: no read or write outside its buffers,
    every output element written, same bits as outside the guard."""
    from test_redzone_gpu import conv_case, run_guarded
    cp = make_conv(c, c, seed=80).cuda()
    call, t = conv_case(cp, epi, n, c, c, h, w)
    run_guarded(call, t, [cp], names=[FORM])
