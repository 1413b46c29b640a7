"""The JPEG round trip on the device (virnet_amd/jpeg.py, csrc/jpeg.hip).  Everything here is an equality of bytes: the arithmetic is
integer, so the device has to reproduce Pillow's libjpeg-turbo (tests/golden/jpeg.npz) and the host definition exactly.  The one bar is
im_blur of ``degrade.synthesize_lr``, which is the blur operator's (tests/test_degrade_gpu.py: k^2 * 2^-23 * the operator on absolute
values, in float64)."""
import glob
import os

import numpy as np
import pytest
import torch

import jpeg_cases
from conftest import GOLDEN
from redzone import guarded
from test_degrade_gpu import _taps64, ref_op
from virnet_amd import _native, degrade, jpeg, sisr_eval
from virnet_amd import eval as veval

pytestmark = pytest.mark.gpu


def nchw(images):
    """list of [h,w,3] arrays -> CUDA [n,3,h,w]"""
    return torch.from_numpy(np.ascontiguousarray(np.stack(images).transpose(0, 3, 1, 2))).cuda()


def hwc(t, i=0):
    return np.ascontiguousarray(t[i].permute(1, 2, 0).cpu().numpy())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def float_images(n, h, w, seed):
    """fp32 in about [-0.1, 1.1] with exact .5/255 ties, zeros, ones and values outside [0,1] in the first rows"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, h, w, generator=g) * 1.2 - 0.1
    ties = (torch.arange(w, dtype=torch.float32) * 3 % 255 + 0.5) / 255.0
    x[:, 0, 0, :] = ties
    x[:, 1, 0, :] = torch.tensor([0.0, 1.0, -0.25, 1.5, -0.0])[torch.arange(w) % 5]
    return x


@pytest.mark.parametrize("h,w", jpeg_cases.sizes())
def test_uint8_equals_libjpeg_byte_for_byte(h, w):
    """every kind at every quality of one size as one batch with a quality per sample, and the first case once more on its own"""
    cases = jpeg_cases.cases(h, w)
    x = nchw([im for _, _, im, _ in cases])
    got = jpeg.jpeg_compress(x, [q for _, q, _, _ in cases])
    assert got.dtype == torch.uint8 and got.shape == x.shape and got.data_ptr() != x.data_ptr()
    for i, (kind, q, im, want) in enumerate(cases):
        diff = int((hwc(got, i) != want).sum())
        assert diff == 0, (h, w, kind, q, diff)
    kind, q, im, want = cases[0]
    assert np.array_equal(hwc(jpeg.jpeg_compress(nchw([im]), q)), want)


@pytest.mark.parametrize("h,w", [(1, 1), (9, 4), (17, 33), (40, 56)])
@pytest.mark.parametrize("q", [1, 40, 100])
def test_float32_equals_the_host_bit_for_bit(h, w, q):
    x = float_images(2, h, w, 7 + h).cuda()
    got = jpeg.jpeg_compress(x, q)
    assert got.dtype == torch.float32 and got.shape == x.shape
    for i in range(2):
        want = veval.jpeg_compress(hwc(x, i), q)
        assert want.dtype == np.float32 and np.array_equal(hwc(got, i).view(np.uint32), want.view(np.uint32)), (h, w, q, i)


@pytest.fixture(scope="module")
def mixed_batch():
    x = float_images(4, 37, 51, 21).cuda()
    return x, [10, 0, 95, 40]


@pytest.mark.parametrize("as_float", [True, False], ids=["float32", "uint8"])
def test_mixed_batch_is_independent_of_the_batch_and_passes_quality_zero_through(mixed_batch, as_float):
    x, qf = mixed_batch
    if not as_float:
        x = (x.clamp(0, 1) * 255).round().to(torch.uint8)
    got = jpeg.jpeg_compress(x, qf)
    for i, q in enumerate(qf):
        assert same_bits(got[i:i + 1], jpeg.jpeg_compress(x[i:i + 1].clone(), q)), i
        want = veval.jpeg_compress(hwc(x, i), q) if q else hwc(x, i)
        assert np.array_equal(hwc(got, i).view(np.uint32 if as_float else np.uint8), want.view(np.uint32 if as_float else np.uint8)), i
    assert same_bits(got[1], x[1])                                              # quality 0: the input's bits, float values not quantised
    assert as_float is False or not same_bits(got[1], jpeg.jpeg_compress(x[1:2], 100)[0])
    # the same call with the qualities as a list, as an int32 tensor, and once more: the same bytes
    qt = torch.tensor(qf, dtype=torch.int32).cuda()
    for other in (jpeg.jpeg_compress(x, qt), jpeg.jpeg_compress(x, tuple(qf)), jpeg.jpeg_compress(x, np.asarray(qf)), jpeg.jpeg_compress(x, qf)):
        assert same_bits(other, got)
    assert same_bits(jpeg.jpeg_compress(x, 40)[3], got[3])


def test_non_contiguous_input_and_no_gradient():
    x = float_images(2, 24, 40, 3).cuda()
    view = x.permute(0, 1, 3, 2)                                                 # [2,3,40,24], not contiguous
    assert same_bits(jpeg.jpeg_compress(view, 75), jpeg.jpeg_compress(view.contiguous(), 75))
    out = jpeg.jpeg_compress(x.clone().requires_grad_(True), 75)
    assert not out.requires_grad and same_bits(out, jpeg.jpeg_compress(x, 75))


def test_graph_capture_replays_the_eager_result(monkeypatch, mixed_batch):
    x, qf = mixed_batch
    x = x.clone()
    qt = torch.tensor(qf, dtype=torch.int32).cuda()
    jpeg.warm(x.device)                                                          # the table is uploaded outside the capture
    want = jpeg.jpeg_compress(x, qt)
    torch.cuda.synchronize()
    streams = []
    real = _native.stream_handle
    monkeypatch.setattr(_native, "stream_handle", lambda: (streams.append(real()), streams[-1])[1])
    graph = torch.cuda.CUDAGraph()
    with _native.capture_lock, torch.cuda.graph(graph):
        capture_stream = torch.cuda.current_stream().cuda_stream
        out = jpeg.jpeg_compress(x, qt)
    monkeypatch.undo()
    assert streams == [capture_stream]                                           # both launches went to the capturing stream: a chain
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, want)
    x.copy_(float_images(4, 37, 51, 22).cuda())                                  # new contents, new qualities: the replay follows them
    qt.copy_(torch.tensor([0, 30, 60, 100], dtype=torch.int32).cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, jpeg.jpeg_compress(x, qt))


def _set5_crop(h, w):
    f = sorted(glob.glob(os.path.join(GOLDEN, "set5", "*.bmp")))[0]
    return veval.img_as_float32(veval.imread_rgb_uint8(f)[16:16 + h, 24:24 + w])


@pytest.mark.parametrize("down", ["bicubic", "direct"])
def test_degrade_lr_with_qf_is_the_round_trip_of_its_own_result(down):
    im = _set5_crop(48, 64)
    kernel = sisr_eval.test_kernels(2)[5]
    plain = degrade.degrade_lr(im, kernel, 2, downsampler=down)
    assert same_bits(plain, degrade.degrade_lr(im, kernel, 2, downsampler=down, qf=None))
    got = degrade.degrade_lr(im, kernel, 2, downsampler=down, qf=40)
    assert got.shape == (1, 3, 24, 32) and got.dtype == torch.float32
    want = veval.jpeg_compress(hwc(plain), 40)
    assert np.array_equal(hwc(got).view(np.uint32), want.view(np.uint32))


def test_sisr_table_passes_qf_through(tmp_path):
    import shutil
    for f in sorted(glob.glob(os.path.join(GOLDEN, "set5", "*.bmp")))[:1]:
        shutil.copy(f, tmp_path)
    seen = []

    def stub(lr, s):
        seen.append(lr)
        lr = hwc(lr) if isinstance(lr, torch.Tensor) else lr
        return np.repeat(np.repeat(lr, s, 0), s, 1)
    kw = dict(kernels=sisr_eval.test_kernels(4)[:1], with_ssim=False)
    sisr_eval.sisr_table(stub, [str(tmp_path) + ":bmp"], 4, device_degrade=True, **kw)
    sisr_eval.sisr_table(stub, [str(tmp_path) + ":bmp"], 4, device_degrade=True, qf=40, **kw)
    plain, lossy = seen
    assert np.array_equal(hwc(lossy).view(np.uint32), veval.jpeg_compress(hwc(plain), 40).view(np.uint32))


@pytest.mark.parametrize("down", ["bicubic", "direct"])
def test_synthesize_lr(down):
    n, hr, sf, k = 3, 48, 2, 21
    g = torch.Generator().manual_seed(31)
    x = torch.from_numpy(np.stack([_set5_crop(hr, hr).transpose(2, 0, 1)] * n)).contiguous()
    x = (x + 0.2 * torch.rand(n, 3, hr, hr, generator=g)).clamp(0, 1.2)           # (some values above 1: the blur's clip acts)
    ker = torch.rand(n, 1, k, k, generator=g) ** 4
    ker = ker / ker.sum((2, 3), keepdim=True)
    noise = torch.randn(n, 3, hr // sf, hr // sf, generator=g)
    std = torch.tensor([2.0, 10.0, 25.0]) / 255.0
    qf = [0, 30, 95]
    im_lr, im_blur = degrade.synthesize_lr(x.cuda(), ker.cuda(), sf, noise.cuda(), std.cuda(), torch.tensor(qf, dtype=torch.int32).cuda(), down)
    assert im_lr.shape == im_blur.shape == (n, 3, hr // sf, hr // sf) and im_lr.dtype == im_blur.dtype == torch.float32
    # im_blur: the clipped blur with the flipped kernel and the symmetric border, downsampled, in float64; the clip is 1-Lipschitz, so
    # the forward operator's bar carries over
    k64 = ker.double().flip(-2, -1)
    blur = ref_op(x.double(), k64, 1, "direct", "symmetric").clamp(0.0, 1.0)
    s_blur = ref_op(x.double().abs(), k64.abs(), 1, "direct", "symmetric")
    if down == "direct":
        ref, s = blur[:, :, ::sf, ::sf], s_blur[:, :, ::sf, ::sf]
    else:
        ref = _taps64(hr, sf) @ blur @ _taps64(hr, sf).t()
        s = _taps64(hr, sf, True) @ s_blur @ _taps64(hr, sf, True).t()
    err = (im_blur.cpu().double() - ref).abs()
    bar = k * k * 2.0 ** -23 * s
    print(f"{down}: im_blur max err {float(err.max()):.3e}, max err/bar {float((err / bar).max()):.3f}")
    assert bool((err <= bar).all())
    # im_lr: the host tail applied to the DEVICE's im_blur, bit for bit
    for i in range(n):
        want = sisr_eval.synthesize_tail_np(hwc(im_blur, i), np.ascontiguousarray(noise[i].permute(1, 2, 0).numpy()), float(std[i]), qf[i])
        assert want.dtype == np.float32 and np.array_equal(hwc(im_lr, i).view(np.uint32), want.view(np.uint32)), i
    # the host function end to end agrees up to the blur's rounding where no JPEG spreads it (sample 0)
    host_lr, host_blur = sisr_eval.synthesize_lr_np(np.ascontiguousarray(x[0].permute(1, 2, 0).numpy()), ker[0, 0].numpy(), sf,
                                                    np.ascontiguousarray(noise[0].permute(1, 2, 0).numpy()), float(std[0]), 0, down)
    assert np.abs(host_blur - hwc(im_blur, 0)).max() <= float(bar[0].max()) * 2 and np.abs(host_lr - hwc(im_lr, 0)).max() <= float(bar[0].max()) * 2 + 2.0 ** -23
    none_lr, none_blur = degrade.synthesize_lr(x.cuda(), ker.cuda(), sf, noise.cuda(), std.cuda(), None, down)
    assert same_bits(none_blur, im_blur) and same_bits(none_lr[0], im_lr[0])


# ---- red zone: no access outside the buffers, every output element written ---------------------------------------------------------------
@pytest.mark.parametrize("as_float", [False, True], ids=["uint8", "float32"])
@pytest.mark.parametrize("h,w", [(1, 1), (17, 33), (40, 56)])
def test_red_zone(h, w, as_float):
    """input, qualities, workspace and output in guarded arenas (tests/redzone.py): no zone is touched, every output element is written, no
    NaN appears, and the result equals the unguarded one.  Quality 0 is in the batch: the copy-through is guarded too.  The workspace
    gets the zone check only (it is exactly virnet_jpeg_workspace_bytes)."""
    x = float_images(3, h, w, 40 + w)
    x = x.cuda() if as_float else (x.clamp(0, 1) * 255).round().to(torch.uint8).cuda()
    qt = torch.tensor([40, 0, 100], dtype=torch.int32).cuda()
    for qf in (qt, 75):
        plain = jpeg.jpeg_compress(x, qf)
        torch.cuda.synchronize()
        with guarded() as g:
            xi = g.input(x)
            out = jpeg.jpeg_compress(xi, g.input(qf) if isinstance(qf, torch.Tensor) else qf)
            g.check(out)
            assert g.home(out) is not None
            sizes = sorted(a.nbytes for a in g.arenas if a.dtype == torch.uint8)
            assert 3 * (h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)) in sizes              # the workspace, at its declared size
        assert same_bits(out, plain)
