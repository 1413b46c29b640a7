"""virnet_amd.param_cache.ParamCache: the one cache of everything derived from parameters -- its key, its eviction rule, and that a copied
or saved module carries no cached value (a ctypes struct of pointers in a module's ``__dict__`` used to make ``copy.deepcopy`` and
``torch.save`` of a network raise after a forward).  Fake builders, no device."""
import copy
import io
import pickle

import torch
from torch import nn

from virnet_amd import _native as nat
from virnet_amd.networks import VIRAttResUNetSR
from virnet_amd.networks.AttResUNet import AttLayer, AttResUNet
from virnet_amd.networks.params import ConvParam
from virnet_amd.param_cache import ParamCache, param_key


class Builder:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def test_hit_returns_the_same_object_and_builds_once():
    cache, build = ParamCache(), Builder()
    w, b = nn.Parameter(torch.zeros(4, 3)), nn.Parameter(torch.zeros(4))
    first = cache.get(("fwd", "wx4"), (w, b), build)
    assert all(cache.get(("fwd", "wx4"), (w, b), build) is first for _ in range(3)) and build.calls == 1
    assert len(cache.slots()) == 1 and cache.slots() == [("fwd", "wx4")]
    assert param_key((w, None, b)) == (id(w), w.data_ptr(), w._version, w.device, None, id(b), b.data_ptr(), b._version, b.device)


def test_every_way_a_parameter_moves_is_a_miss():
    cache, build = ParamCache(), Builder()
    holder = nn.Module()
    holder.w, holder.b = nn.Parameter(torch.zeros(4, 3)), nn.Parameter(torch.zeros(4))
    get = lambda: cache.get(("fwd", "wx4"), (holder.w, holder.b), build)
    seen = [get()]

    def missed():
        seen.append(get())
        return seen[-1] is not seen[-2] and get() is seen[-1] and build.calls == len(seen)

    old = holder.w
    holder.w = nn.Parameter(old.data)                          # another Parameter object on the same storage: only the id moves
    assert holder.w.data_ptr() == old.data_ptr() and holder.w._version == old._version and missed()
    with torch.no_grad():
        holder.w.mul_(2.0)                                     # in-place write: _version moves
    assert missed()
    version = holder.w._version
    holder.w.data = torch.ones(4, 3)                           # new storage, same _version
    assert holder.w._version == version and missed()
    holder.b = None                                            # bias: parameter -> None -> parameter
    assert missed()
    holder.b = nn.Parameter(torch.zeros(4))
    assert missed()


def test_a_slot_is_keyed_on_its_own_parameters_only():
    cache, fwd, dgrad = ParamCache(), Builder(), Builder()
    w, b = nn.Parameter(torch.zeros(4, 3)), nn.Parameter(torch.zeros(4))
    f0, d0 = cache.get(("fwd", "wx4"), (w, b), fwd), cache.get(("dgrad", "wx4"), (w,), dgrad)
    with torch.no_grad():
        b.add_(1.0)                                            # a bias update rebuilds the forward packing, never the input-gradient one
    assert cache.get(("fwd", "wx4"), (w, b), fwd) is not f0 and cache.get(("dgrad", "wx4"), (w,), dgrad) is d0
    assert (fwd.calls, dgrad.calls) == (2, 1)


def test_a_miss_drops_stale_siblings_and_keeps_current_ones():
    cache, build = ParamCache(), Builder()
    w, b = nn.Parameter(torch.zeros(4, 3)), nn.Parameter(torch.zeros(4))
    for form in ("wx4", "direct", "wino"):
        cache.get(("fwd", form), (w, b), build)
    d0 = cache.get(("dgrad", "wx4"), (w,), build)
    assert len(cache.slots()) == 4                                     # a miss among current siblings evicts nothing (the range guard's fp32 re-run)
    with torch.no_grad():
        w.add_(1.0)
    new = cache.get(("fwd", "wx4"), (w, b), build)
    assert set(cache.slots()) == {("fwd", "wx4"), ("dgrad", "wx4")}    # the stale forms of the family went, another family is not this miss's business
    direct = cache.get(("fwd", "direct"), (w, b), build)
    assert set(cache.slots()) == {("fwd", "wx4"), ("fwd", "direct"), ("dgrad", "wx4")} and cache.get(("fwd", "wx4"), (w, b), build) is new
    assert cache.get(("dgrad", "wx4"), (w,), build) is not d0 and cache.get(("fwd", "direct"), (w, b), build) is direct


def test_a_builder_that_declines_stores_and_drops_nothing():
    cache, build = ParamCache(), Builder()
    w = nn.Parameter(torch.zeros(4, 3))
    kept = cache.get(("tail", "wx4"), (w,), build)
    with torch.no_grad():
        w.add_(1.0)
    assert cache.get(("tail", "f16x3"), (w,), lambda: None) is None and set(cache.slots()) == {("tail", "wx4")}
    assert cache.get(("tail", "f16x3"), (w,), build) is not kept and set(cache.slots()) == {("tail", "f16x3")}


def _caches(module):
    return [m._cache for m in module.modules() if isinstance(getattr(m, "_cache", None), ParamCache)]


def _seed(module):
    """an entry in every cache of the module tree -- a real pointer struct in the AttLayers', a tensor elsewhere; {id(cache): the entry}"""
    out = {}
    for m in module.modules():
        cache = getattr(m, "_cache", None)
        if isinstance(cache, ParamCache):
            value = (nat.SftWeights(), []) if isinstance(m, AttLayer) else torch.zeros(1000)
            got = cache.get(("sft",) if isinstance(m, AttLayer) else ("fwd", "wx4"), tuple(m.parameters(recurse=False)), lambda: value)
            assert got is value and len(cache.slots()) == 1
            out[id(cache)] = value
    return out


def _saved(module) -> bytes:
    buf = io.BytesIO()
    torch.save(module, buf)
    return buf.getvalue()


def _sisr():
    return VIRAttResUNetSR(im_chn=3, sigma_chn=1, kernel_chn=3, n_feat=[32, 64], dep_S=2, dep_K=2, n_resblocks=1, noise_cond=True, kernel_cond=True,
                           extra_mode="Both", noise_avg=True)


def test_copies_and_saved_modules_carry_no_cached_value():
    for make, n_caches in ((lambda: AttLayer(32, 4), 5), (lambda: ConvParam(16, 32, 3), 1), (_sisr, None)):
        module = make()
        seeded = _seed(module)
        assert len(seeded) == (n_caches or len(seeded)) and len(seeded) >= 1
        twins = [copy.deepcopy(module), torch.load(io.BytesIO(_saved(module)), weights_only=False), pickle.loads(pickle.dumps(module))]
        for twin in twins:
            assert type(twin) is type(module) and len(_caches(twin)) == len(seeded) and all(len(c.slots()) == 0 for c in _caches(twin))
            assert all(torch.equal(a, b) for a, b in zip(twin.state_dict().values(), module.state_dict().values(), strict=True))
            assert not {id(c) for c in _caches(twin)} & set(seeded)
        for cache in _caches(module):                          # the original keeps its own entries: the same objects as before
            (slot,) = cache.slots()
            assert cache._entries[slot][1] is seeded[id(cache)]
        full = len(_saved(module))
        module.apply(lambda m: getattr(m, "invalidate", lambda: None)())
        assert all(len(c.slots()) == 0 for c in _caches(module)) and len(_saved(module)) == full
    assert any(isinstance(m, AttLayer) for m in _sisr().modules()) and any(isinstance(m, AttResUNet) for m in _sisr().modules())


def test_invalidate_empties_the_cache_of_all_three_owners():
    for module in (ConvParam(16, 32, 3), AttLayer(32, 4), AttResUNet(in_chn=3, extra_chn=1, out_chn=3, n_resblocks=1, n_feat=[32, 64])):
        module._cache.get(("x",), tuple(module.parameters(recurse=False)), object)
        assert len(module._cache.slots()) == 1
        module.invalidate()
        assert len(module._cache.slots()) == 0


def test_conv_param_packs_per_form_with_and_without_a_bias(monkeypatch):
    from virnet_amd import ops
    calls = []
    monkeypatch.setattr(ops, "pack_weight", lambda w, b, **kw: calls.append((b is None, kw)) or object())
    for k in ("VIRNET_CONV_FORM", "VIRNET_WINOGRAD"):
        monkeypatch.delenv(k, raising=False)
    for conv in (ConvParam(8, 16, 3, bias=False), ConvParam(8, 16, 3, stride=2)):
        del calls[:]
        pk = conv.packed()
        assert conv.packed() is pk and conv.packed_dgrad() is conv.packed_dgrad() and conv.packed_dgrad() is not pk
        monkeypatch.setenv("VIRNET_CONV_FORM", "direct")
        assert conv.packed() is not pk and conv.packed() is conv.packed()
        monkeypatch.delenv("VIRNET_CONV_FORM")
        assert conv.packed() is pk and set(conv._cache.slots()) == {("fwd", "wx4"), ("fwd", "direct"), ("dgrad", "wx4")}
        no_bias = conv.bias is None
        assert calls == [(no_bias, dict(transposed=False, stride=conv.stride)), (True, dict(transposed=False, dgrad=True)),
                         (no_bias, dict(transposed=False, stride=conv.stride))]
