"""The red-zone harness (tests/redzone.py) tested on itself: plain torch "ops" on CPU arenas.  No kernel runs, and every access stays
inside the arena the test owns (an "overrun" is a write through a view of that arena).

Each detection test also runs its faulty op with the one check that should catch it switched off and asserts that the fault then goes
unreported: the report comes from that check and from nothing else."""
import os
import re

import numpy as np
import pytest
import torch

import redzone
from redzone import RedZoneError, guarded
from virnet_amd.param_cache import ParamCache

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def good_op(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    return out


def run(op, x, **checks):
    with guarded(cpu=True, **checks) as g:
        out = op(g, g.input(x))
        g.check(out)
    return out


def findings(op, x, **checks):
    with pytest.raises(RedZoneError) as e:
        run(op, x, **checks)
    return e.value.findings


def test_pattern_is_nan_as_fp32_fp16_halves_and_fp64_pairs():
    for p in (redzone.ZONE, redzone.UNWRITTEN):
        assert redzone.pattern_is_nan_everywhere(p)
        w = np.array([p, p], dtype=np.uint32)
        assert np.isnan(w.view(np.float32)).all() and np.isnan(w.view(np.float16)).all() and np.isnan(w.view(np.float64)).all()
        assert len({(p >> s) & 0xFF for s in (0, 8, 16, 24)}) >= 3          # distinctive as an integer, and no run of equal bytes
    assert redzone.ZONE != redzone.UNWRITTEN
    assert not redzone.pattern_is_nan_everywhere(0x7FC00000)                 # (fp32 quiet NaN: its low half is fp16 zero)
    assert not redzone.pattern_is_nan_everywhere(0x7FC5A17E)                 # (not an fp64 NaN)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.float64, torch.uint8, torch.int32, torch.int64])
@pytest.mark.parametrize("shape", [(3, 5), (1,), (7,), (2, 3, 129, 67)])
def test_arena_layout(dtype, shape):
    with guarded(cpu=True) as g:
        e = torch.empty(shape, dtype=dtype, device="cpu")
        z = torch.zeros(*shape, dtype=dtype)
        el, zl = torch.empty_like(e), torch.zeros_like(e, dtype=dtype)
        assert len(g.arenas) == 4
        for t, ar in zip((e, z, el, zl), g.arenas):
            assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and t.data_ptr() % 256 == 0
            assert g.home(t) is ar and ar.tensor.data_ptr() == t.data_ptr() == ar.lo
            nbytes = t.numel() * t.element_size()
            assert ar.nbytes == nbytes and ar.zone % 256 == 0 and ar.zone >= max(nbytes, 256 * 1024)
            front, back = ar.mem[:ar.zone], ar.mem[ar.zone + nbytes:]
            assert front.numel() >= ar.zone and back.numel() >= ar.zone          # the zones start right at the payload's edges
            assert ar.mem.data_ptr() + ar.zone == t.data_ptr()
            assert "test_redzone_host.py" in ar.where and "test_arena_layout" in ar.where
        assert float(z.double().abs().sum()) == 0 and float(zl.double().abs().sum()) == 0
        raw = g.arenas[0].payload_bytes().numpy()
        want = np.frombuffer(np.array([redzone.UNWRITTEN], dtype="<u4").tobytes() * (len(raw) // 4 + 1), dtype=np.uint8)[:len(raw)]
        assert (raw == want).all()
        if dtype.is_floating_point:
            assert bool(torch.isnan(e).all()) and bool(torch.isnan(el).all())
        assert g.arenas[0].unwritten_count(0, len(raw)) == (e.numel() if e.element_size() > 1 else len(raw) // 4 or 1)
        g.check([z, zl])


def test_cpu_and_other_dtypes_pass_through():
    with guarded() as g:                                       # (device arenas only: CPU allocations are not touched)
        a = torch.empty(4)
        b = torch.zeros((2, 2), dtype=torch.float32, device="cpu")
        assert not g.arenas and g.home(a) is None and g.home(b) is None
    with guarded(cpu=True) as g:
        torch.empty(4, dtype=torch.bfloat16)
        torch.zeros(4, dtype=torch.bool)
        torch.empty(4, dtype=torch.int16)
        torch.empty(4, pin_memory=False, requires_grad=False)
        assert len(g.arenas) == 1                              # (defaults spelled out are still a plain allocation)
        out = torch.empty(3)
        torch.empty(3, out=out)
        assert len(g.arenas) == 2


def test_correct_op_passes():
    x = torch.arange(15, dtype=torch.float32).view(3, 5)
    assert torch.equal(run(lambda g, xi: good_op(xi), x), x * 2)


def test_guard_input_is_a_contiguous_copy():
    x = torch.arange(24, dtype=torch.float32).view(2, 3, 4).permute(2, 0, 1)
    with guarded(cpu=True) as g:
        xi = redzone.guard_input(x)
        assert xi.is_contiguous() and xi.shape == x.shape and xi.dtype == x.dtype and torch.equal(xi, x) and g.home(xi) is g.arenas[0]
        with pytest.raises(TypeError):
            g.input(torch.zeros(3, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="outside"):
        redzone.guard_input(x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.uint8])
@pytest.mark.parametrize("side", ["front", "back"])
def test_write_just_outside_the_payload_is_reported(side, dtype):
    x = torch.ones(3, 7, dtype=dtype)                          # (21 elements: an odd byte count for uint8 / fp16 -- the back zone starts unaligned)
    size = x.element_size()

    def op(g, xi):
        out = good_op(xi)
        ar = g.home(out)
        at = ar.zone - size if side == "front" else ar.zone + ar.nbytes
        ar.mem[at:at + size].view(dtype).fill_(3)              # one element just before / just after the payload, inside the arena
        return out

    (f,) = findings(op, x)
    assert f["kind"] == "zone" and f["side"] == side and f["arena"].shape == (3, 7)
    assert (f["first"], f["last"]) == ((-size, -1) if side == "front" else (0, size - 1))
    assert 1 <= f["count"] <= size
    for part in (side + " zone", "(3, 7)", "test_redzone_host.py", "good_op"):
        assert part in f["text"], f["text"]
    run(op, x, check_zones=False)                              # the zone check is what reports it


def test_overrun_is_reported_on_leaving_without_an_explicit_check():
    with pytest.raises(RedZoneError) as e:
        with guarded(cpu=True) as g:
            out = torch.zeros(5)
            g.home(out).mem[g.arenas[0].zone + 20 + 4096] = 0     # far into the back zone, and nobody calls check()
    assert e.value.findings[0]["side"] == "back" and e.value.findings[0]["first"] == 4096


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.float64, torch.int32])
def test_unwritten_element_is_reported(dtype):
    x = torch.arange(15).to(dtype).view(3, 5)

    def op(g, xi):
        out = torch.empty_like(xi)
        out.view(-1)[:14] = xi.view(-1)[:14]                   # skips the last element
        return out

    fs = findings(op, x)
    assert [f["kind"] for f in fs if f["kind"] == "unwritten"] == ["unwritten"] and fs[0]["count"] == 1
    if dtype.is_floating_point:
        fs = findings(op, x, check_unwritten=False)            # a float that was left out still shows as NaN ...
        assert [f["kind"] for f in fs] == ["nan"]
    run(op, x, check_unwritten=False, check_nan=False)         # ... and with both checks off it passes


def test_unwritten_word_of_a_byte_tensor_is_reported():
    x = torch.arange(64, dtype=torch.uint8)

    def op(g, xi):
        out = torch.empty_like(xi)
        out[:8] = xi[:8]
        out[12:] = xi[12:]                                     # bytes 8..11 are skipped
        return out

    (f,) = findings(op, x)
    assert f["kind"] == "unwritten" and f["count"] == 1
    run(op, x, check_unwritten=False)


def test_value_read_from_a_zone_is_reported_through_nan():
    x = torch.ones(4, 4)

    def op(g, xi):
        ar = g.home(xi)
        wide = ar.mem[ar.zone - 4:ar.zone + ar.nbytes].view(torch.float32)      # the input and the element in front of it
        out = torch.empty(4, 4)
        out.view(-1).copy_(wide[1:] + wide[:-1])               # out[0] reads the front zone
        return out

    (f,) = findings(op, x)
    assert f["kind"] == "nan" and f["count"] == 1
    run(op, x, check_nan=False)
    with guarded(cpu=True) as g:                               # a case that expects NaN says so
        g.check(op(g, g.input(x)), allow_nan=True)


def test_result_allocated_outside_the_guard_is_reported():
    x = torch.ones(6)

    def op(g, xi):
        return xi * 2, good_op(xi)                             # (the product comes from torch's own allocator)

    (f,) = findings(op, x)
    assert f["kind"] == "bypass" and f["index"] == 0
    run(op, x, check_home=False)

    def views(g, xi):
        out = good_op(xi)
        return out[2:], out.view(2, 3).t()                     # views of a guarded payload are at home

    run(views, x)


def test_patch_is_removed_after_an_exception():
    orig = {n: getattr(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like")}
    assert not redzone.patch_installed()
    with pytest.raises(KeyError):
        with guarded(cpu=True):
            assert redzone.patch_installed() and torch.empty is not orig["empty"]
            with guarded(cpu=True):                            # nesting: the inner block's exit keeps the outer block's patch
                pass
            assert redzone.patch_installed()
            raise KeyError("boom")
    assert not redzone.patch_installed() and all(getattr(torch, n) is f for n, f in orig.items())
    assert torch.empty(3).data_ptr() and not redzone._ACTIVE


def test_the_guard_covers_every_allocation_route_the_package_uses():
    """tests/redzone.py patches torch.empty / empty_like / zeros / zeros_like.  If the package starts to allocate kernel buffers another
    way (Tensor.new_empty, torch.full, ...), the guard has to learn that route first."""
    other = re.compile(r"\.new_(empty|zeros|ones|full|tensor)\(|torch\.(full|ones|empty_strided|empty_permuted|full_like)\(")
    hits = []
    for root, _, files in os.walk(os.path.join(REPO, "virnet_amd")):
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(root, f)) as fh:
                    hits += [f"{f}:{i}" for i, line in enumerate(fh, 1) if other.search(line)]
    assert hits == []


def test_adopt_moves_parameters_into_arenas_and_restores_them():
    class Owner(torch.nn.Linear):                              # a module with a cache of derived values and the method that drops it
        def invalidate(self):
            self._cache.clear()

    lin = Owner(3, 2)
    before = lin.weight.data_ptr()
    lin._cache = ParamCache()
    assert lin._cache.get(("sft",), (lin.weight, lin.bias), lambda: "stale") == "stale" and len(lin._cache.slots()) == 1
    with guarded(cpu=True) as g:
        g.adopt(lin)
        assert g.home(lin.weight.data) is not None and g.home(lin.bias.data) is not None and len(lin._cache.slots()) == 0
        assert lin.weight.data_ptr() != before
    assert lin.weight.data_ptr() == before
