"""The tensor set and the reference of the weight-average tests (tests/test_ema_gpu.py, tests/test_redzone_ema_gpu.py, tests/test_ema_host.py).

The sizes are those of tests/optim_cases.py (``ALL_SIZES``): around the 16-byte access (1, 3, 4, 5), around a wave and the chunk (255,
CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 1: several workgroups, a tail), the 37-element view at element offset 1 of a 40-element buffer
(4-byte but not 16-byte aligned: the 4-byte access form) and TABLE + 1 further tensors of at most 8 elements, so that a second table is
launched.  Values: parameters ``p`` and averages ``e`` are sign * 10^U(-6, 2); every seventh element has ``p == e`` bitwise (the update's
fixpoint), further elements of either are exact zeros, and tensor ``I_NONFINITE`` holds a NaN with a payload and a +Inf in ``p`` and a -Inf
in ``e`` at known places.

The reference is ``virnet_amd.ema.ema_np`` on CPU copies.  Finite results are compared bit for bit.  Where the reference is NaN (the NaN
itself, and -Inf + Inf) only NaN-ness is compared: IEEE 754 leaves the sign and payload of a NaN that an operation produces to the
implementation, and the host and the device choose differently.  The swap moves words, so there the NaN's bits are compared too."""
import functools

import numpy as np
import torch

import optim_cases as oc

CHUNK, TABLE = oc.CHUNK, oc.TABLE
ALL_SIZES = oc.ALL_SIZES
I_VIEW, VIEW_BUF, VIEW_LEN = oc.I_VIEW, oc.VIEW_BUF, oc.VIEW_LEN
I_NONFINITE = ALL_SIZES.index(255)
NAN_AT, PINF_AT, NINF_AT = 3, 10, 21           # p[NAN_AT] = NaN, p[PINF_AT] = +Inf, e[NINF_AT] = -Inf   (none of them a p == e element)
NAN_BITS = 0x7FC12345                          # a quiet NaN with a payload
NAMES = [f"t{i}" for i in range(len(ALL_SIZES))]
assert len(ALL_SIZES) > TABLE and ALL_SIZES[I_VIEW] == VIEW_LEN


def _draw(n, g):
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 8 - 6)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


@functools.lru_cache(maxsize=None)
def values(seed: int = 0, nonfinite: bool = True):
    """(p, e): two lists of fp32 CPU tensors, one pair per size.  Shared: do not write to them."""
    g = torch.Generator().manual_seed(4000 + seed)
    ps, es = [], []
    for i, n in enumerate(ALL_SIZES):
        p, e = _draw(n, g), _draw(n, g)
        k = torch.arange(n) + i
        p[k % 11 == 5] = 0.0
        e[k % 13 == 6] = 0.0
        same = k % 7 == 3
        e[same] = p[same]
        if nonfinite and i == I_NONFINITE:
            assert not same[[NAN_AT, PINF_AT, NINF_AT]].any()
            p.view(torch.int32)[NAN_AT] = NAN_BITS
            p[PINF_AT] = float("inf")
            e[NINF_AT] = float("-inf")
        ps.append(p)
        es.append(e)
    return ps, es


def fixpoints(i: int) -> torch.Tensor:
    """mask of tensor i's elements that were drawn with p == e"""
    return (torch.arange(ALL_SIZES[i]) + i) % 7 == 3


def make_params(ps, device, wrap=None):
    """(parameters on ``device`` -- the view parameter at element offset 1 of its buffer --, that buffer); ``wrap``: how a CPU tensor
    gets there (default ``.to(device)``)"""
    wrap = wrap or (lambda x: x.to(device))
    view_buf = torch.full((VIEW_BUF,), 0.5)
    view_buf[0], view_buf[-1] = -1.25, 7.75
    view_buf[1:1 + VIEW_LEN] = ps[I_VIEW]
    buf = wrap(view_buf)
    params = [torch.nn.Parameter(buf[1:1 + VIEW_LEN] if i == I_VIEW else wrap(x.clone())) for i, x in enumerate(ps)]
    assert params[I_VIEW].data_ptr() % 16 == 4 or str(device) == "cpu"
    return params, buf


def make_ema(device="cuda", seed: int = 0, nonfinite: bool = True, wrap=None, **kw):
    """(WeightEMA over the set with ``e`` in its shadows, the parameters, the view parameter's buffer)"""
    from virnet_amd.ema import WeightEMA
    ps, es = values(seed, nonfinite)
    params, buf = make_params(ps, device, wrap)
    ema = WeightEMA(list(zip(NAMES, params)), **kw)
    with torch.no_grad():
        for s, e in zip(ema.shadows, es):
            s.copy_(e)
    return ema, params, buf


def bits(t) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def reference_update(es, ps, w):
    """``ema_np`` per tensor on CPU copies -> list of float32 arrays"""
    from virnet_amd.ema import ema_np
    with np.errstate(invalid="ignore", over="ignore"):
        return [ema_np(np.array(e.detach().cpu().numpy()), np.array(p.detach().cpu().numpy()), w) for e, p in zip(es, ps)]


def assert_same(got, want, label=""):
    """``got`` (tensors) against ``want`` (float32 arrays): bitwise where the reference is not NaN, NaN where it is"""
    for i, (g, w) in enumerate(zip(got, want)):
        g = g.detach().cpu().numpy()
        nan = np.isnan(w)
        assert g.shape == w.shape and np.array_equal(np.isnan(g), nan), (label, i, "NaN places differ")
        bad = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)) & ~nan)
        assert bad.size == 0, (label, i, ALL_SIZES[i] if i < len(ALL_SIZES) else None, bad[:8], g[bad[:8]], w[bad[:8]])
