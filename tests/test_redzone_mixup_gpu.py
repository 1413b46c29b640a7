"""MixUp and the real-noise batch under the software red zone (tests/redzone.py): the inputs of ``mixup`` and the pool, table, parameters and
mix of ``real_batch`` entered through ``g.input`` (or allocated by the package inside the guard), the outputs from the package's own
``torch.empty``.  Neither may write outside its outputs, every output element must be written, and no zone value may reach a result.  A
stray READ of the uint8 pool cannot show up as NaN -- the corner crops of tests/datagen_cases.py and the partner's differing crop catch it
by value -- so the outputs are compared with the definitions here too."""
import numpy as np
import pytest
import torch

import datagen_cases as dc
import mixup_cases as mc
from redzone import guarded
from virnet_amd import datagen

pytestmark = pytest.mark.gpu


def _guarded_mix(g, mix):
    dm = mix.to("cuda")                                    # (the buffer comes from torch.empty inside the guard: an arena already)
    assert g.home(dm.blob) is not None
    return dm


@pytest.mark.parametrize("shape", [(9, 3, 20, 20)] + mc.SHAPES, ids=str)
def test_mixup_stays_inside_its_buffers(shape):
    a, b = mc.tensors(shape)
    mix = mc.mix() if shape[0] == 9 else mc.mix_for(shape[0])
    with guarded() as g:
        ta, tb = g.input(torch.from_numpy(np.array(a)).cuda()), g.input(torch.from_numpy(np.array(b)).cuda())
        out = datagen.mixup(ta, tb, _guarded_mix(g, mix))
        g.check(out)
        assert dc.same_bits(out[0], datagen.mixup_np(a, mix)) and dc.same_bits(out[1], datagen.mixup_np(b, mix))


def test_mixup_of_offset_views_stays_inside_its_buffers():
    """both inputs start one element into their payloads (4-byte aligned only); the elements around the views are NaN"""
    shape = (9, 3, 20, 20)
    a, b = mc.tensors(shape)
    count = int(np.prod(shape))
    with guarded() as g:
        views = []
        for v in (a, b):
            buf = torch.full((count + 5,), float("nan"))
            buf[1:1 + count] = torch.from_numpy(np.array(v)).reshape(-1)
            views.append(g.input(buf.cuda())[1:1 + count].view(shape))
        assert all(v.data_ptr() % 16 == 4 for v in views)
        out = datagen.mixup(views[0], views[1], _guarded_mix(g, mc.mix()))
        g.check(out)
        assert dc.same_bits(out[0], datagen.mixup_np(a, mc.mix())) and dc.same_bits(out[1], datagen.mixup_np(b, mc.mix()))


@pytest.mark.parametrize("p", dc.PATCHES)
def test_real_batch_stays_inside_its_buffers(p):
    with guarded() as g:
        pool = datagen.ImagePool.paired(list(dc.images(0)), list(dc.images(1)), "cuda")
        pool.data, pool.table, pool.data_b = g.input(pool.data), g.input(pool.table), g.input(pool.data_b)
        dp = dc.params(p).to("cuda")
        assert g.home(dp.blob) is not None
        out = datagen.real_batch(pool, dp, p, _guarded_mix(g, mc.mix()), 7)
        g.check(out)
        want_noisy, want_gt = mc.expected(p)
        assert dc.same_bits(out[0], want_noisy) and dc.same_bits(out[1], want_gt)
