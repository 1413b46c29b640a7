"""The batch synthesis under the software red zone (tests/redzone.py): pool, table and parameters entered through ``g.input``, the outputs
from the package's own ``torch.empty`` inside the guard.  No mode may write outside its outputs, and every output element must be written.
A stray READ of the uint8 pool cannot show up as NaN; the corner crops of tests/test_datagen_gpu.py catch it by value instead, and the
outputs are compared with the definitions here too."""
import numpy as np
import pytest
import torch

import datagen_cases as dc
from redzone import guarded
from virnet_amd import datagen

pytestmark = pytest.mark.gpu


def _guarded_pool(g, paired=False):
    ims = list(dc.images(0))
    pool = datagen.ImagePool.paired(ims, list(dc.images(1)), "cuda") if paired else datagen.ImagePool(ims, "cuda")
    pool.data, pool.table = g.input(pool.data), g.input(pool.table)
    if paired:
        pool.data_b = g.input(pool.data_b)
    return pool


def _guarded_params(g, params):
    dp = params.to("cuda")                                 # (the blob comes from torch.empty inside the guard: an arena already)
    assert g.home(dp.blob) is not None
    return dp


@pytest.mark.parametrize("drawn", [False, True], ids=["supplied", "drawn"])
@pytest.mark.parametrize("p", dc.PATCHES)
def test_denoise_stays_inside_its_buffers(p, drawn):
    with guarded() as g:
        pool, dp = _guarded_pool(g), _guarded_params(g, dc.params(p))
        noise = None if drawn else g.input(torch.from_numpy(dc.noise(p)).cuda())
        ids = g.input(torch.arange(dc.N, dtype=torch.int64).cuda())
        out = datagen.denoise_batch(pool, dp, p, 7, noise=noise, sample_ids=ids)
        g.check(out)
        assert dc.same_bits(out[1], dc.expected(p)["gt"])
        if not drawn:
            assert np.abs(out[0].cpu().numpy() - dc.expected(p)["noisy"]).max() <= 5e-7


@pytest.mark.parametrize("p", dc.PATCHES)
def test_pair_and_hr_stay_inside_their_buffers(p):
    with guarded() as g:
        pool, dp = _guarded_pool(g, paired=True), _guarded_params(g, dc.params(p))
        a, b = datagen.pair_batch(pool, dp, p)
        hr = datagen.hr_batch(pool, dp, p)
        g.check([a, b, hr])
        want = dc.expected(p)
        assert dc.same_bits(a, want["pair_a"]) and dc.same_bits(b, want["pair_b"]) and dc.same_bits(hr, want["hr"])


@pytest.mark.parametrize("shape", [(3, 1031), (2, 3, 12, 12), (1, 1)])
def test_normal_stays_inside_its_buffer(shape):
    with guarded() as g:
        ids = g.input(torch.arange(shape[0], dtype=torch.int64).cuda())
        g.check(datagen.normal(shape, 7, ids, stream=1))


@pytest.mark.parametrize("k", [1, 21, 25])
def test_blur_kernels_stay_inside_their_buffers(k):
    with guarded() as g:
        rng = np.random.default_rng(k)
        lam = [g.input(torch.from_numpy(rng.uniform(0.05, 16.0, 5)).cuda()) for _ in range(2)]
        theta = g.input(torch.from_numpy(rng.uniform(0, np.pi, 5)).cuda())
        kernel, kinfo = datagen.blur_kernels(lam[0], lam[1], theta, k, 3, True)
        g.check([kernel, kinfo])
