"""Device LPIPS (virnet_amd/lpips.py distance / features, csrc/lpips.hip) against the fp64 definition on the CPU (lpips.distance_torch /
features_torch in float64, tests/lpips_cases.py), never against the device code itself.

The bars come from profiles/lpips_device.md: over every case and both input forms, the float32 torch definition on the CPU deviates from
the float64 one by at most 1.704e-7 (distance, relative) and 8.413e-7 / 6.758e-7 / 6.972e-7 / 5.254e-7 / 6.021e-7 (taps 1..5, max-abs error
over the tap's max).  One fp32 summation order differs from another by about as much as either differs from fp64, so the bar is four times
the measured value: it covers the kernels' blocked k-ordered sums against oneDNN's, not a wrong tap.  What is exact is asserted exactly:
run-to-run bits, batch independence, symmetry, the zero on equal images, uint8 against float32 inputs, eager against a replayed graph."""
import numpy as np
import pytest
import torch

import lpips_cases as lc
from virnet_amd import _native, lpips, sisr_eval
from virnet_amd import eval as veval

pytestmark = pytest.mark.gpu

DIST_F32_VS_F64 = 1.704e-7                                                  # profiles/lpips_device.md, "fp32 against fp64 on the CPU"
TAP_F32_VS_F64 = (8.413e-7, 6.758e-7, 6.972e-7, 5.254e-7, 6.021e-7)
DIST_REL = 4 * DIST_F32_VS_F64
TAP_REL = tuple(4 * v for v in TAP_F32_VS_F64)


def _cuda(case, form):
    a, b = lc.pair(case, form)
    return a.cuda(), b.cuda()


@pytest.mark.parametrize("form", lc.FORMS)
@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_distance_matches_the_fp64_definition(case, form):
    a, b = _cuda(case, form)
    got = lpips.distance(a, b, lc.weights())
    want = lc.reference(case, form)[0]
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (case[2],)
    rel = ((got.cpu() - want).abs() / want).tolist()
    print(f"{case} {form}: device {got.cpu().tolist()} fp64 {want.tolist()} rel {['%.3e' % r for r in rel]} (bar {DIST_REL:.3e})")
    assert max(rel) <= DIST_REL


@pytest.mark.parametrize("form", lc.FORMS)
@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_every_tap_matches_the_fp64_definition(case, form):
    a, _ = _cuda(case, form)
    got = lpips.features(a, lc.weights())
    want = lc.reference(case, form)[1]
    assert len(got) == 5
    errs = []
    for g, r in zip(got, want):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == r.shape and g.is_contiguous()
        errs.append(float((g.cpu().double() - r).abs().max() / r.abs().max()))
    print(f"{case} {form}: tap errors {['%.3e' % e for e in errs]} (bars {['%.3e' % t for t in TAP_REL]})")
    for i, (e, bar) in enumerate(zip(errs, TAP_REL)):
        assert e <= bar, f"tap {i + 1}"
    assert all(float(g.min()) >= 0.0 for g in got)                         # after the ReLU


@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_uint8_and_float32_inputs_give_the_same_bits(case):
    a, b = _cuda(case, "u8")
    w = lc.weights()
    d = lpips.distance(a, b, w)
    fa, fb = a.float() / 255.0, b.float() / 255.0
    assert lc.same_bits(lpips.distance(fa, b, w), d) and lc.same_bits(lpips.distance(a, fb, w), d) and lc.same_bits(lpips.distance(fa, fb, w), d)
    for x, y in zip(lpips.features(a, w), lpips.features(fa, w)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("form", lc.FORMS)
@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_bits_do_not_depend_on_the_run_the_batch_or_the_order(case, form):
    a, b = _cuda(case, form)
    if form == "f32":
        b = b.float() / 255.0                                         # (one dtype per side, so that the sides can be joined below)
    w = lc.weights()
    d = lpips.distance(a, b, w)
    assert lc.same_bits(lpips.distance(a, b, w), d)                                            # run to run
    assert lc.same_bits(lpips.distance(b, a, w), d)                                            # symmetric
    for i in range(case[2]):
        assert lc.same_bits(lpips.distance(a[i:i + 1], b[i:i + 1], w), d[i:i + 1]), i            # alone
    # another place in a larger batch, next to other images
    big_a, big_b = torch.cat([b[:1], a, a[:1]]), torch.cat([a[:1], b, a[:1]])
    big = lpips.distance(big_a, big_b, w)
    assert lc.same_bits(big[1:1 + case[2]], d) and lc.same_bits(big[:1], d[:1])
    assert float(big[-1]) == 0.0 and not np.signbit(float(big[-1]))
    zero = lpips.distance(a, a.clone(), w)
    assert lc.same_bits(zero, torch.zeros(case[2], dtype=torch.float64))                       # exactly +0.0
    assert all(float(v) > 0.0 for v in d)


def test_replay_in_a_captured_graph_equals_the_eager_result():
    case = lc.CASES[2]
    w = lc.weights()
    a, b = _cuda(case, "f32")
    other_a, other_b = _cuda(case, "u8")
    other_a = other_a.float() / 255.0
    eager = lpips.distance(a, b, w)                                  # (warm: the weights are packed and nothing is loaded while capturing)
    eager_other = lpips.distance(other_a, other_b, w)
    sa, sb = a.clone(), b.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _native.capture_lock, torch.cuda.graph(graph):
        out = lpips.distance(sa, sb, w)
    for xa, xb, want in ((a, b, eager), (other_a, other_b, eager_other), (a, b, eager)):
        sa.copy_(xa)
        sb.copy_(xb)
        graph.replay()
        torch.cuda.synchronize()
        assert lc.same_bits(out, want)
    assert not lc.same_bits(eager, eager_other)


def test_enqueues_on_the_current_stream():
    case = lc.CASES[3]
    w = lc.weights()
    a, b = _cuda(case, "u8")
    d = lpips.distance(a, b, w)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        again = lpips.distance(a, b, w)
    s.synchronize()
    assert lc.same_bits(again, d)


def test_sisr_table_device_lpips_matches_the_host_path(tmp_path):
    from PIL import Image
    dst = tmp_path / "synth"
    dst.mkdir()
    for i, case in enumerate(((66, 80, 1), (71, 65, 1))):
        Image.fromarray(np.ascontiguousarray(lc.pair_u8(case)[0][0].numpy().transpose(1, 2, 0))).save(str(dst / f"im{i}.bmp"))
    spec = str(dst) + ":bmp"
    w = lc.weights()
    sf = 2
    kernels = sisr_eval.test_kernels(sf)[:2]

    def host_forward(lr, sf_):
        return np.repeat(np.repeat(lr, sf_, axis=0), sf_, axis=1) * np.float32(1.1) - np.float32(0.05)

    def device_forward(lr, sf_):
        t = torch.from_numpy(np.ascontiguousarray(lr.transpose(2, 0, 1)[np.newaxis])).cuda()
        return t.repeat_interleave(sf_, dim=2).repeat_interleave(sf_, dim=3) * 1.1 - 0.05

    host = sisr_eval.sisr_table(host_forward, [spec], sf, kernels=kernels, lpips=w)
    dev = sisr_eval.sisr_table(device_forward, [spec], sf, kernels=kernels, device_metrics=True, lpips=w)
    plain = sisr_eval.sisr_table(device_forward, [spec], sf, kernels=kernels, device_metrics=True)
    for h, d, p in zip(host, dev, plain):
        assert list(d) == list(h) == list(p) + ["lpips", "per_image_lpips"]
        assert {k: d[k] for k in p} == p and d["per_image_psnr_y"] == h["per_image_psnr_y"]            # same uint8 SR image on both paths
        assert len(d["per_image_lpips"]) == 2 and all(type(v) is float for v in d["per_image_lpips"])
        for f, x, y in zip(sorted(str(q) for q in dst.iterdir()), d["per_image_lpips"], h["per_image_lpips"]):
            # the yardstick is the fp64 definition on the same uint8 images; the host column is the float32 definition
            gt = sisr_eval.modcrop(veval.imread_rgb_uint8(f), sf)
            sr = veval.img_as_ubyte(np.clip(host_forward(sisr_eval.degrade(veval.img_as_float32(gt), kernels[d["kernel"] - 1], sf), sf), 0.0, 1.0))
            ta, tb = (torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[None])) for im in (sr, gt))
            ref = float(lpips.distance_torch(ta, tb, w, torch.float64)[0])
            print(f"kernel {d['kernel']}: device {x:.9f} host {y:.9f} fp64 {ref:.9f}")
            assert abs(x - ref) <= DIST_REL * ref and abs(y - ref) <= DIST_REL * ref
        assert d["lpips"] == float(np.mean(d["per_image_lpips"]))
