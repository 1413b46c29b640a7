"""Gradient buckets on the device (csrc/gradsync.hip, virnet_amd.dist.pack_grads / unpack_grads) and the GradientReducer built on them, in
one process.  Every comparison is bit for bit against the torch expressions the reducer used before: ``bucket[off:off+n].copy_(g).mul_(s)``
going in, ``bucket[off:off+n].clone().mul_(s)`` coming out.  The tensor set (tests/gradsync_cases.py) is built once per module."""
import pytest
import torch

import gradsync_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def cases():
    tensors, sizes, view_buf, fill_buf = gc.make_tensors(DEV)
    offsets, length = gc.make_offsets(sizes)
    return dict(tensors=tensors, sizes=sizes, offsets=offsets, length=length, view_buf=view_buf, fill_buf=fill_buf)


def _sentinel(length):
    return torch.full((length,), gc.SENTINEL, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0, 0.125], ids=["1", "1/2", "1/3", "1/8"])
def test_pack_matches_copy_mul(cases, scale):
    from virnet_amd import dist as vdist
    want = _sentinel(cases["length"])
    for t, off, n in zip(cases["tensors"], cases["offsets"], cases["sizes"]):
        if t is None:
            want[off:off + n].zero_()
        else:
            want[off:off + n].copy_(t.reshape(-1)).mul_(scale)
    got = _sentinel(cases["length"])
    launches = vdist.pack_grads(cases["tensors"], cases["offsets"], got, scale, sizes=cases["sizes"])
    assert launches == 2                                              # TABLE + 1 entries: the second launch ran
    assert torch.equal(gc.bits(got), gc.bits(want))                   # slots, the null slot's zeros, and every sentinel word between and after
    off, n = cases["offsets"][gc.I_NULL], gc.NULL_LEN
    assert not gc.bits(got[off:off + n]).any()
    covered = torch.zeros(cases["length"], dtype=torch.bool)
    for off, n in zip(cases["offsets"], cases["sizes"]):
        covered[off:off + n] = True
    assert int((~covered).sum()) > len(cases["sizes"]) and bool((got.cpu()[~covered] == gc.SENTINEL).all())
    off = cases["offsets"][gc.I_SPECIAL]
    special = got[off + 1:off + 4].cpu()
    assert torch.isnan(special[0]) and special[1] == float("inf") and special[2] == float("-inf")
    if scale == 1.0 / 3.0:                                            # a real rounding: the product is not the exact third
        src = cases["tensors"][3].double().cpu()
        off = cases["offsets"][3]
        assert bool((got[off:off + 64].double().cpu() != src / 3.0).any())


def _bucket(cases):
    gen = torch.Generator().manual_seed(5)
    b = (torch.rand(cases["length"], generator=gen) - 0.5).to(DEV)
    off = cases["offsets"][gc.I_SPECIAL]
    b[off + 1:off + 4] = torch.tensor([float("nan"), float("inf"), float("-inf")], device=DEV)
    return b


@pytest.mark.parametrize("in_place", [False, True], ids=["fresh", "in_place"])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -7], ids=["1", "2^-7"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host_scale", "device_scale"])
def test_unpack_matches_clone_mul(cases, scale, in_place, on_device):
    from virnet_amd import dist as vdist
    bucket = _bucket(cases)
    before = gc.bits(bucket)
    live = [i for i, t in enumerate(cases["tensors"]) if t is not None]
    offsets = [cases["offsets"][i] for i in live]
    want = [bucket[cases["offsets"][i]:cases["offsets"][i] + cases["sizes"][i]].clone().mul_(scale) for i in live]
    if in_place:                                                      # existing gradients: the set's own layout, the odd view included
        tensors, _, view_buf, fill_buf = gc.make_tensors(DEV, seed=3)
        outs = [tensors[i] for i in live]
        edges = (gc.bits(view_buf[:1]), gc.bits(view_buf[1 + gc.VIEW_LEN:]))
    else:
        outs = [torch.empty(cases["sizes"][i], dtype=torch.float32, device=DEV) for i in live]
    s = torch.tensor([scale], dtype=torch.float32, device=DEV) if on_device else scale
    assert vdist.unpack_grads(bucket, offsets, outs, s) == 1          # TABLE live entries: one launch
    for i, o, w in zip(live, outs, want):
        assert torch.equal(gc.bits(o), gc.bits(w)), f"tensor {i} ({cases['sizes'][i]} elements at offset {cases['offsets'][i]})"
    assert torch.equal(gc.bits(bucket), before)
    if in_place:
        assert torch.equal(gc.bits(view_buf[:1]), edges[0]) and torch.equal(gc.bits(view_buf[1 + gc.VIEW_LEN:]), edges[1])
    k = live.index(gc.I_SPECIAL)
    special = outs[k][1:4].cpu()
    assert torch.isnan(special[0]) and special[1] == float("inf") and special[2] == float("-inf")


def test_non_contiguous_tensors_are_made_contiguous():
    from virnet_amd import dist as vdist
    g = torch.arange(24.0, device=DEV).reshape(4, 6).t()
    bucket = _sentinel(30)
    vdist.pack_grads([g], [3], bucket, 0.5)
    assert torch.equal(bucket[3:27], g.contiguous().reshape(-1) * 0.5) and float(bucket[2]) == gc.SENTINEL and float(bucket[27]) == gc.SENTINEL
    out = torch.zeros(6, 4, device=DEV).t()
    vdist.unpack_grads(bucket, [3], [out], 2.0)
    assert torch.equal(out.contiguous().reshape(-1), g.contiguous().reshape(-1))


# ---- the reducer, world 1 (no process group) ------------------------------------------------------------------------------------------
SHAPES = [(8, 3, 3, 3), (8,), (16, 8, 3, 3), (16,), (5,), (1,)]       # 216, 8, 1152, 16, 5, 1 elements


def _params():
    gen = torch.Generator().manual_seed(11)
    return [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in SHAPES]


def _grads(params, step):
    gen = torch.Generator().manual_seed(100 + step)
    return [torch.randn(p.shape, generator=gen).to(DEV) for p in params]


class _Counter:
    def __init__(self, monkeypatch):
        from virnet_amd import _native
        self.calls = {"pack": 0, "unpack": 0}
        lib = _native.load()
        for key in self.calls:
            real = getattr(lib, "virnet_gradsync_" + key)
            monkeypatch.setattr(lib, "virnet_gradsync_" + key, self._wrap(key, real))

    def _wrap(self, key, real):
        def call(*args):
            self.calls[key] += 1
            return real(*args)
        return call

    def take(self):
        out = (self.calls["pack"], self.calls["unpack"])
        self.calls = {"pack": 0, "unpack": 0}
        return out


def _parent_finish(params, pushed, bucket_elems, unscale):
    """What the reducer computed before the device buckets, written out: zeroed buckets in the given layout, ``copy_().mul_(1 / world)`` per
    pushed gradient, ``clone().view_as(p)`` per parameter, then the backward's ``_foreach_mul_`` by its un-scale factor."""
    out = []
    for p in params:
        b = torch.zeros(bucket_elems, dtype=torch.float32, device=DEV)          # (slot position does not change a copy's bits)
        if id(p) in pushed:
            b[3:3 + p.numel()].copy_(pushed[id(p)].reshape(-1)).mul_(1.0)
        out.append(b[3:3 + p.numel()].clone().view_as(p))
    torch._foreach_mul_(out, unscale)
    return out


@pytest.mark.parametrize("skip_one", [False, True], ids=["all_pushed", "one_never_pushed"])
def test_reducer_push_finish_matches_parent_expressions(monkeypatch, skip_one):
    from virnet_amd import dist as vdist
    params = _params()
    red = vdist.GradientReducer(params, bucket_bytes=2048)                        # 512 floats: several buckets
    count = _Counter(monkeypatch)
    unscale = torch.tensor(2.0 ** -5, dtype=torch.float32, device=DEV)
    for step in range(3):                                                         # step 0 on the guessed layout, then the observed one
        grads = _grads(params, step)
        calls = [[5, 4], [3, 2], [1, 0]]                                          # back to front, a conv's weight and bias per call
        if skip_one:
            calls[0] = [5]
        red.begin_step()
        red.start()
        for idx in calls:
            red.push({params[i]: grads[i] for i in idx})
        n_pack, _ = count.take()
        assert n_pack == 3                                                        # one pack per push call, whatever buckets it touched
        out = red.finish(unscale.reshape(1))
        n_pack, n_unpack = count.take()
        n_buckets = len(red.bucket_sizes) if step else n_unpack                   # (step 0's finish re-lays the buckets after unpacking)
        assert n_pack == (1 if skip_one else 0) and n_unpack == n_buckets and n_unpack >= 2
        assert red.consumed
        pushed = {id(params[i]): grads[i] for idx in calls for i in idx}
        want = _parent_finish(params, pushed, 2048, unscale)
        for p, w in zip(params, want):
            assert out[p].shape == p.shape and out[p].is_contiguous()
            assert torch.equal(gc.bits(out[p]), gc.bits(w)), (step, tuple(p.shape))
        if skip_one:
            assert not gc.bits(out[params[4]]).any()
        assert all(out[p].data_ptr() < red._flat.data_ptr() or out[p].data_ptr() >= red._flat.data_ptr() + 4 * red._flat.numel() for p in params)


def test_reducer_finish_default_unscale_is_identity(monkeypatch):
    from virnet_amd import dist as vdist
    params = _params()
    red = vdist.GradientReducer(params)
    grads = _grads(params, 0)
    red.start()
    red.push(dict(zip(params, grads)))
    out = red.finish()
    for p, g in zip(params, grads):
        assert torch.equal(gc.bits(out[p]), gc.bits(g))


def test_reduce_grads_world1_is_identity_and_keeps_none(monkeypatch):
    from virnet_amd import dist as vdist
    params = _params()
    red = vdist.GradientReducer(params, bucket_bytes=2048)
    count = _Counter(monkeypatch)
    grads = _grads(params, 7)
    for i, (p, g) in enumerate(zip(params, grads)):
        p.grad = None if i == 3 else g.clone()
    held = [p.grad for p in params]
    red.begin_step()
    assert not red.consumed
    red.ensure_reduced()
    n_buckets = len(red.bucket_sizes)
    assert count.take() == (n_buckets, n_buckets) and n_buckets >= 2 and red.consumed
    for i, (p, g) in enumerate(zip(params, grads)):
        if i == 3:
            assert p.grad is None
        else:
            assert p.grad is held[i]                                              # written in place
            assert torch.equal(gc.bits(p.grad), gc.bits(g))
    red.ensure_reduced()                                                          # already averaged this step: nothing runs
    assert count.take() == (0, 0)
    red.begin_step()
    red.ensure_reduced()
    assert count.take() == (n_buckets, n_buckets)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from virnet_amd import dist as vdist
    bucket = torch.zeros(64, device=DEV)
    ok = torch.ones(8, device=DEV)
    with pytest.raises(TypeError, match="float32"):
        vdist.pack_grads([ok, torch.ones(8, device=DEV, dtype=torch.float16)], [0, 8], bucket, 1.0)
    with pytest.raises(TypeError, match="float32"):
        vdist.unpack_grads(bucket, [0], [torch.ones(8, device=DEV, dtype=torch.float16)], 1.0)
    with pytest.raises(ValueError, match="is on cpu"):
        vdist.pack_grads([ok, torch.ones(8)], [0, 8], bucket, 1.0)
    with pytest.raises(ValueError, match="is on cpu"):
        vdist.unpack_grads(bucket, [0, 8], [ok, torch.ones(8)], 1.0)
    with pytest.raises(ValueError, match="beyond the bucket"):
        vdist.pack_grads([ok], [57], bucket, 1.0)
    with pytest.raises(ValueError, match="beyond the bucket"):
        vdist.unpack_grads(bucket, [-1], [ok], 1.0)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        vdist.pack_grads([torch.ones(8)], [0], torch.zeros(64), 1.0)
    with pytest.raises(TypeError, match="float32"):
        vdist.pack_grads([ok], [0], bucket.double(), 1.0)
    with pytest.raises(ValueError, match="sizes"):
        vdist.pack_grads([None], [0], bucket, 1.0)
    assert not gc.bits(bucket).any()                                              # a refused call launched nothing
    # the library checks the slots itself
    import ctypes as C
    from virnet_amd import _native
    lib = _native.load()
    rc = lib.virnet_gradsync_pack((C.c_void_p * 1)(ok.data_ptr()), (C.c_longlong * 1)(8), (C.c_longlong * 1)(57), 1, bucket.data_ptr(), 64, 1.0,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"beyond the bucket" in lib.virnet_last_error()
