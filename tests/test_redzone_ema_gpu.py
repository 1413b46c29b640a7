"""The weight average under the software red zone (tests/redzone.py): the tensor set of tests/ema_cases.py, every parameter in a guarded
arena, the shadows from the package's own ``empty_like`` inside the guard.  A chunk's tail, the 4-byte access form of the view parameter
and the second table must neither read nor write outside their tensors, in the update and in the swap."""
import numpy as np
import pytest
import torch

import ema_cases as ec
from redzone import guarded
from virnet_amd.ema import weight_at

pytestmark = pytest.mark.gpu


def _guarded_ema(g, **kw):
    n_before = len(g.arenas)
    ema, params, buf = ec.make_ema("cuda", wrap=lambda x: g.input(x.cuda()), **kw)
    assert len(g.arenas) == n_before + 2 * len(params)                           # every parameter (the view's buffer once) and every shadow
    assert g.home(buf) is not None and g.home(params[ec.I_VIEW].data) is g.home(buf) and params[ec.I_VIEW].data_ptr() % 16 == 4
    assert all(g.home(s) is not None for s in ema.shadows)
    return ema, params, buf


def _check(g, tensors):
    """zones intact; every tensor at home, fully written and -- the one with the NaN aside, which keeps exactly its own -- free of NaN"""
    g.check([t for i, t in enumerate(tensors) if i != ec.I_NONFINITE])
    g.check([tensors[ec.I_NONFINITE]], allow_nan=True)


def test_update_stays_inside_its_tensors():
    with guarded() as g:
        ema, params, buf = _guarded_ema(g, decay=0.9)
        ps, es = ec.values(0)
        edge = (ec.bits(buf[0]), ec.bits(buf[1 + ec.VIEW_LEN:]))
        n_before = len(g.arenas)
        ema.update()
        assert len(g.arenas) == n_before                                         # no workspace
        _check(g, ema.shadows)
        _check(g, [p.data for p in params])
        assert np.flatnonzero(np.isnan(ema.shadows[ec.I_NONFINITE].cpu().numpy())).tolist() == sorted((ec.NAN_AT, ec.NINF_AT))
        assert np.array_equal(ec.bits(buf[0]), edge[0]) and np.array_equal(ec.bits(buf[1 + ec.VIEW_LEN:]), edge[1])
        assert all(np.array_equal(ec.bits(p), ec.bits(q)) for p, q in zip(params, ps))          # the parameters are not written
        ec.assert_same(ema.shadows, ec.reference_update(es, ps, weight_at(0, 0.9)), "guarded update")


def test_swap_stays_inside_its_tensors():
    with guarded() as g:
        ema, params, buf = _guarded_ema(g, decay=0.9)
        ps, es = ec.values(0)
        edge = (ec.bits(buf[0]), ec.bits(buf[1 + ec.VIEW_LEN:]))
        n_before = len(g.arenas)
        ema.swap()
        assert len(g.arenas) == n_before
        _check(g, ema.shadows)
        _check(g, [p.data for p in params])
        assert np.array_equal(ec.bits(buf[0]), edge[0]) and np.array_equal(ec.bits(buf[1 + ec.VIEW_LEN:]), edge[1])
        assert all(np.array_equal(ec.bits(p), ec.bits(e)) for p, e in zip(params, es))
        assert all(np.array_equal(ec.bits(s), ec.bits(p)) for s, p in zip(ema.shadows, ps))
        ema.swap()
        _check(g, ema.shadows)
        _check(g, [p.data for p in params])
        assert all(np.array_equal(ec.bits(p), ec.bits(q)) for p, q in zip(params, ps))
