"""The composed tail (engine.rnet_forward): the last up-path block's conv2 composed at pack time with the tail's taps-as-rows
GEMM (ops.compose_exit_weight), run as a 96 -> 32 conv whose map the exit kernel adds to A x (virnet_conv_exit_add).  The reference of
every accuracy case is torch on the CPU in fp64 computing the TWO-STEP definition  out = crop(tail(r + conv2(t) + b2)) + x_in  -- never
the composed path's own output.

Bars.  Operator level: the project's per-conv bar, 2e-5 relative to the output's largest magnitude (tests/test_conv_wx4_gpu.py), and at most
twice the present two-launch path's error on the same inputs (both printed before the assertion; profiles/tail_compose.md has them).
Whole net, default against VIRNET_TAIL_COMPOSE=0: 2e-5 absolute on mu (the documented agreement between conv forms, ops.wx4_shape_ok),
sigma bit for bit.  Against the fp64 oracle after a weight update: 1e-3, the bar smoke() holds the whole net to -- the updates scale a
weight by 1.5, which moves mu by far more (asserted), so a stale image cannot pass."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from virnet_amd import _native as nat
from virnet_amd import engine, graph, ops
from virnet_amd.networks import VIRAttResUNet, VIRAttResUNetSR
from virnet_amd.utils.synth import synth_images, synth_state_dict
from test_ops_gpu import make_conv, nhwc, rnd
from test_redzone_gpu import run_guarded

pytestmark = pytest.mark.gpu
TOL = 2e-5
CFG = dict(n_feat=[96, 192, 288], dep_S=5, n_resblocks=3, noise_cond=True, extra_mode="Input", noise_avg=False)
SR_CFG = dict(im_chn=3, sigma_chn=1, kernel_chn=3, n_feat=[96, 160, 224], dep_S=5, dep_K=8, noise_cond=True, kernel_cond=True,
              n_resblocks=2, extra_mode="Both", noise_avg=True)
WX4_OPEN = {"VIRNET_WX4_MIN_TILES": "0", "VIRNET_WX4_MIN_FILL": "0", "VIRNET_WX4_MIN_WGS": "0"}     # the Winograd form at test sizes


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("VIRNET_CONV_FORM", "VIRNET_WINOGRAD", "VIRNET_TAIL_COMPOSE", "VIRNET_TAIL_COMPOSE_FORM", "VIRNET_EXIT_FORM", "VIRNET_DETERMINISTIC",
              "VIRNET_WX4_MIN_COUT"):
        monkeypatch.delenv(k, raising=False)


def _ceil4(v):
    return (v + 3) // 4 * 4


class Layers:
    def __init__(self, seed=3):
        self.conv2 = make_conv(96, 96, seed=seed).cuda()
        self.tail = make_conv(96, 3, seed=seed + 10).cuda()
        assert float(self.conv2.bias.detach().abs().min()) > 0 and float(self.tail.bias.detach().abs().min()) > 0


def _inputs(n, h, w, sf=1, seed=20):
    """(r, t NCHW cpu on the padded size, x_in NCHW cpu at low resolution, crop)"""
    H, W = h * sf, w * sf
    Hp, Wp = _ceil4(H), _ceil4(W)
    return rnd(n, 96, Hp, Wp, seed=seed), rnd(n, 96, Hp, Wp, seed=seed + 1), rnd(n, 3, h, w, seed=seed + 2), (H, W)


def ref64(L, r, t, x_in, crop, sf):
    w2, b2, we, be = (p.detach().cpu().double() for p in (L.conv2.weight, L.conv2.bias, L.tail.weight, L.tail.bias))
    y = r.double() + F.conv2d(t.double(), w2, b2, padding=1)
    out = F.conv2d(y, we, be, padding=1)[:, :, :crop[0], :crop[1]]
    return out + F.interpolate(x_in.double(), scale_factor=sf, mode="nearest")


def two_launch(L, r, t, x_in, crop, sf):
    y, _ = ops.conv_mfma(t, L.conv2.packed(), res=r, want_raw=True)
    return ops.conv_planar(y, L.tail, crop, op=nat.NCHW_ADD, res=x_in, res_sf=sf)


def composed(L, r, t, x_in, crop, sf, thin_wx4=True, parts=False):
    pw = ops.compose_exit_weight(L.conv2.weight, L.conv2.bias, L.tail.weight)
    z_c, _ = ops.conv_mfma(t, pw, want_raw=True, thin_wx4=thin_wx4)
    out = ops.conv_f16_nchw(r, L.tail.packed(), crop, op=nat.NCHW_ADD, res=x_in, res_sf=sf, z_add=z_c)
    return (z_c, out) if parts else out


class ConvForms:
    """the form of every ops.conv_mfma launch inside the block"""

    def __enter__(self):
        self.forms, self._real = [], ops._launch_conv

        def spy(d, flops, what, form="direct", te=None):
            self.forms.append(form)
            return self._real(d, flops, what, form, te)
        ops._launch_conv = spy
        return self

    def __exit__(self, *exc):
        ops._launch_conv = self._real
        return False


def _check(L, n, h, w, sf, form, monkeypatch, capsys):
    if form == "wx4":
        for k, v in WX4_OPEN.items():
            monkeypatch.setenv(k, v)
    r, t, x_in, crop = _inputs(n, h, w, sf)
    ref = ref64(L, r, t, x_in, crop, sf)
    rg, tg, xg = nhwc(r), nhwc(t), x_in.cuda()
    e_two = float((two_launch(L, rg, tg, xg, crop, sf).cpu().double() - ref).abs().max())
    with ConvForms() as rec:
        got = composed(L, rg, tg, xg, crop, sf, thin_wx4=form == "wx4").cpu().double()
    assert rec.forms == [form], rec.forms
    err = (got - ref).abs()
    scale = float(ref.abs().max())
    e_comp = float(err.max())
    corners = [float(err[:, :, y, x].max()) for y in (0, -1) for x in (0, -1)]
    edge = float(err[:, :, 0, :].max())
    with capsys.disabled():
        print(f"\ntail_compose {n}x{h}x{w} sf{sf} {form}: two-launch {e_two:.3e} composed {e_comp:.3e} (scale {scale:.2f}, bar {TOL * scale:.3e}) "
              f"corners {max(corners):.3e} top row {edge:.3e}")
    assert e_comp <= TOL * scale, (e_comp, TOL * scale)
    assert e_comp <= 2 * e_two, (e_comp, e_two)
    assert all(c <= TOL * scale for c in corners), corners          # (a bias folded as a scalar or a 5x5 shortcut goes wrong here first)
    assert edge <= TOL * scale, edge


@pytest.fixture(scope="module")
def layers():
    return Layers()


@pytest.mark.parametrize("form", ["f16x3", "wx4"])
@pytest.mark.parametrize("n,h,w", [(2, 19, 37), (1, 16, 32), (2, 40, 72)])
def test_composed_tail_against_fp64(layers, n, h, w, form, monkeypatch, capsys):
    """cropped with ragged tiles and border taps / exactly one exit tile / several tiles; 96 channels, non-zero b2 and tail bias"""
    _check(layers, n, h, w, 1, form, monkeypatch, capsys)


@pytest.mark.parametrize("form", ["f16x3", "wx4"])
@pytest.mark.parametrize("h,w,sf", [(8, 12, 2), (5, 7, 3)])
def test_composed_tail_with_nearest_upsampled_residual(layers, h, w, sf, form, monkeypatch, capsys):
    """`+ x_in` through nearest x sf (the SISR exit): LR 8 x 12 x2, and an odd size x3 (15 x 21 cropped out of 16 x 24)"""
    _check(layers, 1, h, w, sf, form, monkeypatch, capsys)


def test_composed_weight_is_the_fp64_composition(layers):
    """virnet_compose_exit_weight: rows (c, tap) of A w2 and A b2 formed in fp64 and rounded once (within half a unit in the last place
    of the fp64 value, bar one-neighbour ties on under 0.1 % of the entries); rows 27..31 zero"""
    L = layers
    wc = torch.empty((32, 96, 3, 3), device="cuda")
    bc = torch.empty(32, device="cuda")
    nat.check(nat.load().virnet_compose_exit_weight(nat.ptr(L.conv2.weight), nat.ptr(L.conv2.bias), nat.ptr(L.tail.weight), 3, 96, 96, nat.ptr(wc),
                                                    nat.ptr(bc), nat.stream_handle()), "compose")
    A = L.tail.weight.detach().cpu().double().permute(0, 2, 3, 1).reshape(27, 96)          # [c*9 + t][m]
    ref_w = torch.einsum("rm,mik->rik", A, L.conv2.weight.detach().cpu().double().reshape(96, 96, 9)).reshape(27, 96, 3, 3)
    ref_b = A @ L.conv2.bias.detach().cpu().double()
    # (the fp64 sums run in another order than torch's: the rounded values may differ where a sum sits on a rounding boundary, by one
    #  neighbour at the most -- an fp32 accumulation is off by several units in the cancelling entries)
    for got, ref in ((wc[:27].cpu().double(), ref_w), (bc[:27].cpu().double(), ref_b)):
        assert bool(((got - ref).abs() <= ref.abs() * 2.0 ** -23).all())
        assert float(((got - ref).abs() > ref.abs() * 2.0 ** -24).double().mean()) < 1e-3
    assert not bool(wc[27:].any()) and not bool(bc[27:].any())


def _rnet_net(seed=0):
    net = VIRAttResUNet(im_chn=3, sigma_chn=1, **CFG)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=seed)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


def test_knob_off_is_the_two_existing_launches_bit_for_bit(monkeypatch):
    """VIRNET_TAIL_COMPOSE=0: the forward's last two launches are conv_mfma(t, conv2, res=r) and conv_planar(y, tail) -- repeated here by
    hand on the recorded operands, bit for bit -- and nothing asks for an additive map; with the default the exit gets one"""
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")
    net, _ = _rnet_net()
    rnet = net.RNet
    x = synth_images(2, 3, 19, 37).cuda()
    sig = torch.rand(2, 1, 19, 37, device="cuda") * 0.1 + 0.01
    calls = {"mfma": [], "planar": [], "z_add": 0}
    real_mfma, real_planar, real_nchw = ops.conv_mfma, ops.conv_planar, ops.conv_f16_nchw

    def spy_mfma(x_, pw, **kw):
        out = real_mfma(x_, pw, **kw)
        calls["mfma"].append((x_, pw, kw, out))
        return out

    def spy_planar(x_, conv, crop, **kw):
        calls["planar"].append((x_, conv, crop, kw))
        return real_planar(x_, conv, crop, **kw)

    def spy_nchw(*a, **kw):
        calls["z_add"] += kw.get("z_add") is not None
        return real_nchw(*a, **kw)
    monkeypatch.setattr(ops, "conv_mfma", spy_mfma)
    monkeypatch.setattr(ops, "conv_planar", spy_planar)
    monkeypatch.setattr(ops, "conv_f16_nchw", spy_nchw)
    with torch.no_grad():
        monkeypatch.setenv("VIRNET_TAIL_COMPOSE", "0")
        out = engine.rnet_forward(rnet, x, extra_map=sig, map_sqrt=True)
        assert calls["z_add"] == 0 and len(calls["planar"]) == 1
        t, pw, kw, (y, _) = calls["mfma"][-1]
        blk = rnet.up_path[-1].body[-1]
        assert pw is blk.conv2.packed() and kw.get("res") is not None and calls["planar"][0][0] is y and calls["planar"][0][1] is rnet.tail
        y2, _ = real_mfma(t, blk.conv2.packed(), res=kw["res"], want_raw=True)
        out2 = real_planar(y2, rnet.tail, (19, 37), op=nat.NCHW_ADD, res=x, res_sf=1)
        assert torch.equal(y2, y) and torch.equal(out2, out)
        monkeypatch.delenv("VIRNET_TAIL_COMPOSE")
        out3 = engine.rnet_forward(rnet, x, extra_map=sig, map_sqrt=True)
        assert calls["z_add"] == 1 and len(calls["planar"]) == 1
        assert float((out3 - out).abs().max()) <= TOL
        with torch.enable_grad():                                                    # grad mode keeps the two launches
            engine.rnet_forward(rnet, x, extra_map=sig, map_sqrt=True)
        assert calls["z_add"] == 1 and len(calls["planar"]) == 2


def test_deterministic_mode_is_batch_independent(monkeypatch):
    """VIRNET_DETERMINISTIC=1: one image alone and the same image inside a batch of 3 agree bit for bit (composition on)"""
    monkeypatch.setenv("VIRNET_DETERMINISTIC", "1")
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")
    net, _ = _rnet_net()
    x = synth_images(3, 3, 40, 56).cuda()
    with torch.no_grad():
        mu3, sig3 = net(x)
        mu1, sig1 = net(x[1:2].contiguous())
    assert torch.equal(mu3[1:2], mu1) and torch.equal(sig3[1:2], sig1)


def test_stale_weights_are_never_used(monkeypatch):
    """in-place update of conv2.weight, then of tail.weight, of conv2.bias, then a .cpu().cuda() round trip: the next forwards -- eager and from the
    automatic graph replay -- match a fresh fp64 reference of the NEW weights"""
    net, _ = _rnet_net(seed=2)
    blk = net.RNet.up_path[-1].body[-1]
    x = synth_images(1, 3, 24, 40)
    xg = x.cuda()

    def ref():
        sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
        return cpu_ref.virnet_denoise(sd, x.double(), **CFG)[0]

    def forwards():
        with torch.no_grad():
            outs = [net(xg)[0].clone() for _ in range(graph.AUTO_AFTER + 2)]            # eager, eager, capture + replay, replay
        return outs[0], outs[-1]

    before = ref()
    for o in forwards():
        assert float((o.cpu().double() - before).abs().max()) <= 1e-3
    assert graph.auto_stats(net)["replays"] >= 2
    last = before
    for step in ("conv2", "tail", "bias", "roundtrip"):
        with torch.no_grad():
            if step == "conv2":
                blk.conv2.weight.mul_(1.5)
            elif step == "tail":
                net.RNet.tail.weight.mul_(1.5)
            elif step == "bias":
                blk.conv2.bias.add_(0.5)
            else:
                net = net.cpu().cuda()                                                  # (new storage, same values and versions)
        now = ref()
        assert step == "roundtrip" or float((now - last).abs().max()) > 1e-2, step      # (the update is far outside the bar below)
        replays = graph.auto_stats(net)["replays"]
        for o in forwards():
            assert float((o.cpu().double() - now).abs().max()) <= 1e-3, step
        assert graph.auto_stats(net)["replays"] >= replays + 2, step
        last = now


def test_range_guard_sees_t_and_the_forward_returns_the_fp32_rerun(layers, monkeypatch):
    """an activation t beyond fp16's range raises the flag in the composed conv (y is never staged; t and r still are); a forward that
    overflows returns the fp32 re-run's result -- bit for bit the fp32 forms' forward, and the oracle's to the guard tests' 1e-3"""
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")
    L = layers
    r, t, x_in, crop = _inputs(1, 16, 32)
    t[0, 5, 7, 9] = 7.0e4
    flag = ops.range_flag(torch.device("cuda", torch.cuda.current_device()))
    flag.zero_()
    composed(L, nhwc(r), nhwc(t), x_in.cuda(), crop, 1, thin_wx4=False)
    assert ops.range_overflowed(flag.device)
    t[0, 5, 7, 9] = 0.5
    r[0, 5, 7, 9] = 7.0e4
    composed(L, nhwc(r), nhwc(t), x_in.cuda(), crop, 1, thin_wx4=False)
    assert ops.range_overflowed(flag.device)
    composed(L, nhwc(rnd(1, 96, 16, 32)), nhwc(t), x_in.cuda(), crop, 1, thin_wx4=False)
    assert not ops.range_overflowed(flag.device)

    net, sd = _rnet_net()
    x = synth_images(1, 3, 64, 64)
    x[0, :, 20:24, 20:24] = 3.0e4                      # (tests/test_guard_gpu.py: the head conv amplifies this beyond fp16's range inside RNet)
    xg = x.cuda()
    with torch.no_grad():
        with ops.forward_scope(form=engine.FP32_FORM):
            ref32 = [o.clone() for o in engine._denoise_forward(net, xg)]
        with pytest.warns(RuntimeWarning, match="fp16's range"):
            mu, sigma = net(xg)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            net(synth_images(1, 3, 64, 64).cuda())
    assert torch.equal(mu, ref32[0]) and torch.equal(sigma, ref32[1])
    mu_ref = cpu_ref.virnet_denoise(sd, x, **CFG)[0]
    assert float((mu.cpu() - mu_ref).abs().max()) <= 1e-3 * max(1.0, float(mu_ref.abs().max()))


def test_composed_pair_in_red_zones():
    """the composed launch pair at 2 x 19 x 37 between guard zones: z_c, r, t, x_in, the weights, the composed images and out"""
    L = Layers(seed=5)
    r, t, x_in, crop = _inputs(2, 19, 37)

    def call(r, t, x_in):
        return composed(L, r, t, x_in, crop, 1, thin_wx4=False, parts=True)
    run_guarded(call, dict(r=nhwc(r), t=nhwc(t), x_in=x_in.cuda()), [L.conv2, L.tail])


def _ab(monkeypatch, fwd):
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")
    count = {"z_add": 0}
    real = ops.conv_f16_nchw

    def spy(*a, **kw):
        count["z_add"] += kw.get("z_add") is not None
        return real(*a, **kw)
    monkeypatch.setattr(ops, "conv_f16_nchw", spy)
    with torch.no_grad():
        on = [o.clone() for o in fwd()]
        assert count["z_add"] == 1
        monkeypatch.setenv("VIRNET_TAIL_COMPOSE", "0")
        off = [o.clone() for o in fwd()]
        assert count["z_add"] == 1
    return on, off


def test_whole_denoise_net_default_against_knob_off(monkeypatch):
    net, _ = _rnet_net()
    x = synth_images(1, 3, 40, 56).cuda()
    (mu, sigma), (mu0, sigma0) = _ab(monkeypatch, lambda: net(x))
    assert float((mu - mu0).abs().max()) <= TOL
    assert torch.equal(sigma, sigma0)                   # SNet is untouched


def test_whole_sr_net_default_against_knob_off(monkeypatch):
    net = VIRAttResUNetSR(**SR_CFG)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=5), strict=True)
    net = net.cuda().eval()
    x = synth_images(1, 3, 16, 24).cuda()
    (mu, kinfo, sigma), (mu0, kinfo0, sigma0) = _ab(monkeypatch, lambda: net(x, 4))
    assert mu.shape == (1, 3, 64, 96)
    assert float((mu - mu0).abs().max()) <= TOL
    assert torch.equal(sigma, sigma0) and torch.equal(kinfo, kinfo0)
