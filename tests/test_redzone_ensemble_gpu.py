"""The self-ensemble kernels under the software red zone (tests/redzone.py), on the partial-tile and non-square cases: sources and restored
groups enter through ``g.input``, the outputs come from the package's own ``torch.empty`` inside the guard.  Nothing may be written outside
an output and every output element must be written.  A stray READ of a uint8 source cannot show up as NaN (tests/test_redzone_datagen_gpu.py
has the same note); the comparison with the definitions catches it by value."""
import pytest
import torch

import ensemble_cases as ec
from redzone import guarded
from virnet_amd import ensemble

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("case", ec.EDGE_CASES, ids=ec.EDGE_IDS)
def test_expand_stays_inside_its_buffers(case, dtype):
    src = ec.source_u8(case) if dtype == "u8" else ec.source_f32(case)
    with guarded() as g:
        dev = g.input(torch.from_numpy(src.copy()).cuda())
        got = ensemble.expand(dev)
        plain = ensemble.expand(dev, flip=False)
        g.check([got.even, got.odd, plain.even])
        want = ec.expanded(case, dtype)
        assert got.batch is None and ec.same_bits(got.even, want[0]) and ec.same_bits(got.odd, want[1])
        assert ec.same_bits(plain.even, ec.expanded(case, dtype, False)[0])


def test_square_expand_writes_both_halves_of_its_one_buffer():
    case = (32, 32, 3, 3)
    with guarded() as g:
        got = ensemble.expand(g.input(torch.from_numpy(ec.source_u8(case).copy()).cuda()))
        g.check(got.batch)
        assert len([a for a in g.arenas if a.dtype == torch.float32]) == 1
        want = ec.expanded(case, "u8")
        assert ec.same_bits(got.even, want[0]) and ec.same_bits(got.odd, want[1])


@pytest.mark.parametrize("case", ec.EDGE_CASES, ids=ec.EDGE_IDS)
def test_reduce_stays_inside_its_buffers(case):
    with guarded() as g:
        even, odd = (g.input(torch.from_numpy(a.copy()).cuda()) for a in ec.restored(case))
        first = g.input(even[:case[3]])
        for order, out, layout in ec.OPTIONS:
            got = ensemble.reduce(even, odd, order=order, out=out, layout=layout)
            plain = ensemble.reduce(first, None, order=order, out=out, layout=layout)
            g.check([got, plain])
            assert ec.same_bits(got, ec.reduced(case, order, out, layout)), (order, out, layout)
            assert ec.same_bits(plain, ec.reduced(case, order, out, layout, False)), (order, out, layout, "noflip")
