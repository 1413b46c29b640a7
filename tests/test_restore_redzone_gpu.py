"""The tiled-restoration kernels under the software red zone (tests/redzone.py), on the smallest plans of tests/restore_cases.py: sources,
restored stacks and the plan's tap tables enter through ``g.input``, the outputs come from the package's own ``torch.empty`` inside the
guard.  Nothing may be written outside an output, every output element must be written, and no zone may be read into a result (a float
zone word is a NaN; a stray READ of a uint8 source cannot show up as NaN, the comparison with the definitions catches it by value)."""
import pytest
import torch

import restore_cases as rc
from redzone import guarded
from virnet_amd import restore

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_gather_stays_inside_its_buffers(case):
    p, want = rc.plan_of(case), rc.gathered(case)
    with guarded() as g:
        src = g.input(torch.from_numpy(rc.image(case).copy()).cuda())
        whole = restore.gather(src, p, 0, p.T, layout=case[5])
        last = restore.gather(src, p, p.T - 1, p.T, layout=case[5])              # the box that ends at the image's last byte
        first = restore.gather(src, p, 0, 1, layout=case[5])
        g.check([whole, last, first])
        assert rc.same_bits(whole, want) and rc.same_bits(last, want[-1:]) and rc.same_bits(first, want[:1])


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("case", rc.BLEND_CASES, ids=rc.BLEND_IDS)
def test_blend_stays_inside_its_buffers(case, scale):
    for blend in restore.BLENDS:
        p = restore.plan(case[1], case[2], case[6], case[7], scale=scale, blend=blend, channels=case[3])      # (a plan of this test's own)
        with guarded() as g:
            tiles = g.input(torch.from_numpy(rc.stack(case, scale).copy()).cuda())
            p.adopt_tables(g.input(torch.from_numpy(p.table_blob()).cuda()))
            for out, layout in rc.OPTIONS:
                got = restore.blend(tiles, p, out=out, layout=layout)
                g.check(got)
                assert rc.same_bits(got, rc.blended(case, scale, blend, out, layout)), (blend, out, layout)
            raw = restore.blend(tiles, p, out="float32", layout="hwc", clip=False)
            g.check(raw)


def test_restore_tiles_writes_every_stack_element():
    case = rc.CASES[0]
    p = rc.plan_of(case, 2)
    with guarded() as g:
        src = g.input(torch.from_numpy(rc.image(case).copy()).cuda())
        stacks = restore.restore_tiles(lambda t: (t.repeat_interleave(2, 2).repeat_interleave(2, 3), t[:, :1].repeat_interleave(2, 2).repeat_interleave(2, 3) + 1),
                                       src, p, batch=5)
        g.check(list(stacks))
        want = rc.gathered(case).repeat(2, axis=2).repeat(2, axis=3)
        assert rc.same_bits(stacks[0], want) and rc.same_bits(stacks[1], want[:, :1] + 1)
