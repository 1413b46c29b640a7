"""The device optimizer under the software red zone (tests/redzone.py): the tensor set of tests/optim_cases.py, every parameter and
gradient in a guarded arena, the moments from the package's own ``zeros_like`` inside the guard.  A chunk's tail, the 4-byte access form
of the view parameter and the second table must neither read nor write outside their tensors."""
import pytest
import torch

import optim_cases as oc
from redzone import guarded

pytestmark = pytest.mark.gpu


def _guarded_params(g):
    wrap = lambda x: g.input(x.cuda())
    params, buf = oc.make_params(1, "cuda", wrap=wrap)
    assert g.home(buf) is not None and g.home(params[oc.I_VIEW].data) is g.home(buf) and params[oc.I_VIEW].data_ptr() % 16 == 4
    oc.set_grads(params, 0, wrap=wrap)
    return params, buf


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_step_stays_inside_its_tensors():
    with guarded() as g:
        params, buf = _guarded_params(g)
        edge = (_bits(buf[0]), _bits(buf[1 + oc.VIEW_LEN:]))
        opt = oc.clip_adam(params)
        n_before = len(g.arenas)
        opt.step()
        stepped = [p for i, p in enumerate(params) if i != oc.I_NOGRAD]
        moments = [opt.state[p][k] for p in stepped for k in ("exp_avg", "exp_avg_sq")]
        assert len(g.arenas) >= n_before + len(moments) + 2          # the moments, the workspace and the norms were allocated inside the guard
        assert params[oc.I_NOGRAD] not in opt.state
        # zones intact; every result at home, written and free of NaN (a zone or an unwritten word read into p, m, v or the norms shows here)
        g.check([p.data for p in stepped] + moments + [opt.grad_norms, opt.clip_coefs] + [p.grad for p in stepped])
        assert torch.equal(_bits(buf[0]), edge[0]) and torch.equal(_bits(buf[1 + oc.VIEW_LEN:]), edge[1])
        ref, tor = oc.fp64_run(1, [0]), oc.torch_run(1, [0])
        oc.check_bound(oc.state_lists(opt, params), tor, ref, "guarded step")


def test_clip_grad_norm_stays_inside_its_tensors():
    from virnet_amd.optim import clip_grad_norm_
    with guarded() as g:
        params, buf = _guarded_params(g)
        before = [_bits(p) for p in params]
        whole = _bits(buf)
        norms = [clip_grad_norm_(oc.members(params, s), oc.MAX_NORMS[s]) for s in (0, 1)]
        g.check(norms + [p.grad for p in params if p.grad is not None])
        assert all(torch.equal(_bits(p), b) for p, b in zip(params, before)) and torch.equal(_bits(buf), whole)      # parameters are not touched
        want = oc.fp64_run(1, [0])["norms"][0]
        assert all(abs(float(n) - w) <= oc.ulp(w) for n, w in zip(norms, want))
