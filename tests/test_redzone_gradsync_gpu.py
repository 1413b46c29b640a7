"""The gradient-bucket kernels under the software red zone (tests/redzone.py): the tensor set of tests/gradsync_cases.py with every tensor,
the view's buffer, the fillers' buffer and the bucket in guarded arenas.  A slot's scalar head and tail, the 4-byte loads of a source whose
phase differs from its slot's and the second table must neither read nor write outside their tensors."""
import pytest
import torch

import gradsync_cases as gc
from redzone import UNWRITTEN, guarded

pytestmark = pytest.mark.gpu


def _set(g):
    tensors, sizes, view_buf, fill_buf = gc.make_tensors("cuda", wrap=g.input)
    assert g.home(view_buf) is not None and g.home(tensors[gc.I_VIEW]) is g.home(view_buf) and g.home(tensors[-1]) is g.home(fill_buf)
    offsets, length = gc.make_offsets(sizes)
    return tensors, sizes, offsets, length


def test_pack_stays_inside_its_tensors():
    from virnet_amd import dist as vdist
    with guarded() as g:
        tensors, sizes, offsets, length = _set(g)
        tensors[gc.I_SPECIAL][1:4] = 0.25                      # (no NaN of the set's own: a NaN in the bucket then came from a zone)
        before = [None if t is None else gc.bits(t) for t in tensors]
        bucket = torch.empty(length, dtype=torch.float32, device="cuda")          # an arena: the unwritten pattern everywhere
        assert g.home(bucket) is not None
        assert vdist.pack_grads(tensors, offsets, bucket, 1.0 / 3.0, sizes=sizes) == 2
        slots = [bucket[off:off + n] for off, n in zip(offsets, sizes)]
        g.check(slots)                                         # zones intact; every slot written, none holds a NaN
        assert all(b is None or torch.equal(gc.bits(t), b) for t, b in zip(tensors, before))      # sources untouched
        covered = torch.zeros(length, dtype=torch.bool)
        for off, n in zip(offsets, sizes):
            covered[off:off + n] = True
        assert bool((gc.bits(bucket)[~covered] == UNWRITTEN).all())      # words between and after the slots were not written
        for t, s in zip(tensors, slots):
            if t is None:
                assert not gc.bits(s).any()
            else:
                assert torch.equal(gc.bits(s), gc.bits(t.reshape(-1).clone().mul_(1.0 / 3.0)))


def test_unpack_stays_inside_its_tensors():
    from virnet_amd import dist as vdist
    with guarded() as g:
        tensors, sizes, offsets, length = _set(g)
        gen = torch.Generator().manual_seed(5)
        bucket = g.input((torch.rand(length, generator=gen) - 0.5).cuda())
        whole = gc.bits(bucket)
        live = [i for i, t in enumerate(tensors) if t is not None]
        scale = g.input(torch.tensor([2.0 ** -7], device="cuda"))
        # in place: the set's own tensors (the view at 4 mod 16, the fillers back to back at every phase)
        outs = [tensors[i] for i in live]
        assert vdist.unpack_grads(bucket, [offsets[i] for i in live], outs, scale) == 1
        g.check(outs)
        # fresh tensors from the allocation route the reducer uses
        fresh = [torch.empty(sizes[i], dtype=torch.float32, device="cuda") for i in live]
        vdist.unpack_grads(bucket, [offsets[i] for i in live], fresh, 2.0 ** -7)
        g.check(fresh)
        assert torch.equal(gc.bits(bucket), whole)
        for i, o, f in zip(live, outs, fresh):
            want = bucket[offsets[i]:offsets[i] + sizes[i]].clone().mul_(2.0 ** -7)
            assert torch.equal(gc.bits(o), gc.bits(want)) and torch.equal(gc.bits(f), gc.bits(want)), i
