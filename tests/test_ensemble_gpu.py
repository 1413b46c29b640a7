"""The self-ensemble kernels (csrc/ensemble.hip) against their numpy definitions (virnet_amd/ensemble.py), bit for bit, on the shared
cases of tests/ensemble_cases.py; then the whole path around the real-noise network against the host loop it replaces."""
import numpy as np
import pytest
import torch

import ensemble_cases as ec
from virnet_amd import _native, ensemble, real_eval
from virnet_amd import eval as veval

pytestmark = pytest.mark.gpu

_NETS = {}


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared cases are read-only)


def _source(case, dtype):
    return ec.source_u8(case) if dtype == "u8" else ec.source_f32(case)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("case", ec.CASES, ids=ec.IDS)
def test_expand_equals_the_definition_bit_for_bit(case, dtype):
    h, w, c, b = case
    src = _source(case, dtype)
    got = ensemble.expand(src)                                        # a numpy array is uploaded
    again = ensemble.expand(_cuda(src))                               # a CUDA tensor is used as it is
    want = ec.expanded(case, dtype)
    for g in (got, again):
        assert ec.same_bits(g.even, want[0]) and ec.same_bits(g.odd, want[1])
        assert g[0] is g.even and g[1] is g.odd and g.even.is_contiguous() and g.odd.is_contiguous()
    if h == w:                                                        # square: two halves of one tensor, nothing to concatenate
        assert got.batch.shape == (8 * b, c, h, w) and got.batch.is_contiguous()
        assert got.even.data_ptr() == got.batch.data_ptr() and got.odd.data_ptr() == got.batch[4 * b:].data_ptr()
        assert ec.same_bits(got.batch, np.concatenate(want))
    else:
        assert got.batch is None
    plain = ensemble.expand(src, flip=False)
    assert plain.odd is None and plain.batch is plain.even and ec.same_bits(plain.even, ec.expanded(case, dtype, False)[0])


@pytest.mark.parametrize("case", ec.CASES, ids=ec.IDS)
def test_reduce_equals_the_definition_bit_for_bit(case):
    even, odd = (_cuda(a) for a in ec.restored(case))
    first = even[:case[3]].contiguous()
    for order, out, layout in ec.OPTIONS:
        got = ensemble.reduce(even, odd, order=order, out=out, layout=layout)
        assert ec.same_bits(got, ec.reduced(case, order, out, layout)), (order, out, layout)
        got = ensemble.reduce(first, None, order=order, out=out, layout=layout)                  # modes = 1: no flip
        assert ec.same_bits(got, ec.reduced(case, order, out, layout, False)), (order, out, layout, "noflip")


def test_the_two_orders_differ_on_the_device_too():
    case = (36, 52, 3, 3)
    even, odd = (_cuda(a) for a in ec.restored(case))
    seq = ensemble.reduce(even, odd, order="sequential", out="float32")
    pair = ensemble.reduce(even, odd, order="pairwise", out="float32")
    assert int((seq != pair).sum()) >= 100


@pytest.mark.parametrize("case", [(5, 3, 3, 3), (32, 32, 1, 3), (33, 31, 3, 3), (64, 96, 3, 3)], ids=lambda c: "x".join(map(str, c)))
def test_an_image_does_not_depend_on_its_batch_and_calls_repeat(case):
    for dtype in ("u8", "f32"):
        src = _cuda(_source(case, dtype))
        whole = ensemble.expand(src)
        twice = ensemble.expand(src)
        assert torch.equal(whole.even.view(torch.int32), twice.even.view(torch.int32))
        assert torch.equal(whole.odd.view(torch.int32), twice.odd.view(torch.int32))
        for i in range(case[3]):
            one = ensemble.expand(src[i:i + 1])
            assert torch.equal(one.even.view(torch.int32), whole.even[4 * i:4 * i + 4].view(torch.int32))
            assert torch.equal(one.odd.view(torch.int32), whole.odd[4 * i:4 * i + 4].view(torch.int32))
    even, odd = (_cuda(a) for a in ec.restored(case))
    for order, out, layout in ec.OPTIONS:
        whole = ensemble.reduce(even, odd, order=order, out=out, layout=layout)
        twice = ensemble.reduce(even, odd, order=order, out=out, layout=layout)
        as_bits = (lambda t: t.view(torch.int32)) if out == "float32" else (lambda t: t)
        assert torch.equal(as_bits(whole), as_bits(twice))
        for i in range(case[3]):
            one = ensemble.reduce(even[4 * i:4 * i + 4], odd[4 * i:4 * i + 4], order=order, out=out, layout=layout)
            assert torch.equal(as_bits(one[0]), as_bits(whole[i]))


@pytest.mark.parametrize("case", ec.CASES, ids=ec.IDS)
def test_expand_identity_reduce_returns_the_source_bytes(case):
    src = ec.source_u8(case)
    dev = _cuda(src)
    for order in ensemble.ORDERS:
        assert torch.equal(ensemble.reduce(*ensemble.expand(dev), order=order), dev)
        assert torch.equal(ensemble.restore(lambda x: x, src, order=order, batch=3), dev)         # chunks that split a source's octet
    assert torch.equal(ensemble.restore(lambda x: x, dev, flip=False), dev)
    assert torch.equal(ensemble.restore(lambda x: x, dev, layout="chw"), dev.permute(0, 3, 1, 2))
    got = ensemble.restore(lambda x: x, dev, order="pairwise", out="float32")                    # (eight equal values: this mean is exact)
    assert got.is_cuda and ec.same_bits(got, np.float32(src / 255.0))


def test_restore_refuses_a_forward_that_changes_the_shape():
    with pytest.raises(ValueError, match="same shape"):
        ensemble.restore(lambda x: x[:, :1], ec.source_u8((5, 3, 3, 1)))
    with pytest.raises(ValueError, match="same shape"):
        ensemble.restore(lambda x: x.cpu(), ec.source_u8((5, 3, 3, 1)))


def test_both_calls_in_one_captured_graph_follow_the_source():
    case = (36, 52, 3, 3)
    first, second = ec.source_u8(case), np.ascontiguousarray(ec.source_u8(case)[::-1, :, ::-1])
    src = _cuda(first)
    ensemble.reduce(*ensemble.expand(src))                           # (warm: nothing is loaded for the first time while capturing)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _native.capture_lock, torch.cuda.graph(graph):
        groups = ensemble.expand(src)
        back = ensemble.reduce(*groups, order="sequential", out="uint8", layout="hwc")
        mean = ensemble.reduce(*groups, order="pairwise", out="float32", layout="chw")
    for source in (first, second):
        src.copy_(_cuda(source))
        graph.replay()
        torch.cuda.synchronize()
        want = ensemble.expand(_cuda(source))                         # the eager result
        assert torch.equal(groups.even, want.even) and torch.equal(groups.odd, want.odd)
        assert ec.same_bits(groups.even, ensemble.expand_np(source)[0])
        assert torch.equal(back, _cuda(source)) and torch.equal(back, ensemble.reduce(*want))
        assert torch.equal(mean, ensemble.reduce(*want, order="pairwise", out="float32", layout="chw"))
    assert not np.array_equal(first, second)


# ---- around the real-noise network --------------------------------------------------------------------------------------------------
def _real_net(manifest):
    if "real" not in _NETS:
        from virnet_amd.networks import VIRAttResUNet
        from virnet_amd.utils.synth import synth_state_dict
        cfg = dict(manifest["configs"]["real"]); cfg.pop("kind")
        net = VIRAttResUNet(**cfg)
        net.load_state_dict(synth_state_dict({k: tuple(s) for k, s in manifest["shapes"]["real"].items()}), strict=True)
        _NETS["real"] = net.cuda().eval()
    return _NETS["real"]


def _n1(net):
    """numpy [n,3,h,w] -> numpy [n,3,h,w] through one N = 1 forward per image: the parent path's launches."""
    def forward(x):
        with torch.no_grad():
            return np.concatenate([net(_cuda(x[i:i + 1]))[0].cpu().numpy() for i in range(len(x))])
    return forward


def _host_loop(net, block_u8):
    """(eval.flip_ensemble of the block, the eight restorations turned back) with N = 1 forwards fed np.float32(u / 255.0)."""
    back = []

    def hwc(a):
        return _n1(net)(np.ascontiguousarray(a.transpose(2, 0, 1))[np.newaxis])[0].transpose(1, 2, 0)

    def recording(mode_input):
        out = hwc(mode_input)
        back.append(veval.dihedral_inverse(out, len(back)))
        return out

    mean = veval.flip_ensemble(recording, np.float32(block_u8 / 255.0))
    return mean, back


def _device_forward(net):
    def forward(x):
        with torch.no_grad():
            return net(x)[0]
    return forward


def test_restore_equals_the_host_loop_of_single_image_forwards(manifest, monkeypatch):
    """36 x 52, the `real` configuration.  With the kernel forms pinned (VIRNET_DETERMINISTIC=1: an image's result does not depend on its
    batch, tests/test_e2e_gpu.py, tests/test_tail_compose_gpu.py) the batched device path gives the host loop's bytes."""
    net = _real_net(manifest)
    block = ec.source_u8((36, 52, 3, 1))
    fwd = _device_forward(net)
    monkeypatch.setenv("VIRNET_DETERMINISTIC", "1")
    mean, back = _host_loop(net, block[0])
    got = ensemble.restore(fwd, block, out="uint8")
    assert got.is_cuda and got.shape == (1, 36, 52, 3)
    assert np.array_equal(got.cpu().numpy()[0], veval.img_as_ubyte(np.clip(mean, 0, 1)))
    inside = float(((mean > 0) & (mean < 1)).mean())
    print(f"distinct bytes {len(np.unique(got.cpu().numpy()))}, share of means inside (0,1) {inside:.3f}")
    assert len(np.unique(got.cpu().numpy())) >= 64                         # (not a comparison of saturated images: 246 values, 16 % inside)
    stack =np.zeros((36, 52, 3, 8), dtype=np.float32)                # dnd_submission_py/pytorch_wrapper.py:19-33 on the same forwards
    for m in range(8):
        stack[:, :, :, m] = back[m]
    want = np.clip(stack.mean(axis=3, keepdims=False), 0.0, 1.0)
    assert ec.same_bits(ensemble.restore(fwd, block, order="pairwise", out="float32")[0], want)
    assert ec.same_bits(torch.from_numpy(real_eval.dnd_box(net, np.float32(block[0] / 255.0))), want)
    # no flip: img_as_ubyte(clip(net(x)[0]))
    x = np.ascontiguousarray(np.float32(block[0] / 255.0).transpose(2, 0, 1))[np.newaxis]
    plain = _n1(net)(x)[0].transpose(1, 2, 0)
    assert np.array_equal(ensemble.restore(fwd, block, flip=False).cpu().numpy()[0], veval.img_as_ubyte(plain.clip(0, 1)))
    assert ec.same_bits(torch.from_numpy(real_eval.dnd_box(net, np.float32(block[0] / 255.0), flip=False)), np.clip(plain, 0.0, 1.0))


def test_restore_is_close_to_the_host_loop_under_the_default_rules(manifest):
    """Default launch rules: single images may take another kernel form than a batch of four, so closeness, at the bar
    tests/test_eval_extras.py holds this ensemble to."""
    net = _real_net(manifest)
    block = ec.source_u8((36, 52, 3, 1))
    mean, _ = _host_loop(net, block[0])
    got = ensemble.restore(_device_forward(net), block, out="float32").cpu().numpy()[0]
    err = float(np.abs(got - np.clip(mean, 0.0, 1.0)).max())
    print(f"max-abs difference to the host loop: {err:.3e}")
    assert err <= 1e-4


def test_sidd_blocks_equals_the_host_table(manifest, monkeypatch):
    net = _real_net(manifest)
    rng = np.random.default_rng(9)
    gt = rng.integers(0, 256, size=(1, 2, 32, 32, 3), dtype=np.uint8)
    noisy = np.clip(gt.astype(np.int32) + rng.integers(-25, 26, size=gt.shape), 0, 255).astype(np.uint8)
    monkeypatch.setenv("VIRNET_DETERMINISTIC", "1")
    want = real_eval.sidd_blocks_np(_n1(net), noisy, gt)
    for batch in (8, 16, 3):
        got = real_eval.sidd_blocks(net, noisy, gt, batch=batch)
        assert got["denoised"].dtype == np.uint8 and np.array_equal(got["denoised"], want["denoised"])
        assert got["psnr"].shape == (1, 2) and np.array_equal(got["psnr"], want["psnr"]) and got["psnr_mean"] == want["psnr_mean"]
        assert float(np.abs(got["ssim"] - want["ssim"]).max()) <= 1e-10 and abs(got["ssim_mean"] - want["ssim_mean"]) <= 1e-10
    plain = real_eval.sidd_blocks(net, noisy, flip=False)
    assert set(plain) == {"denoised"}
    assert np.array_equal(plain["denoised"], real_eval.sidd_blocks_np(_n1(net), noisy, flip=False)["denoised"])
