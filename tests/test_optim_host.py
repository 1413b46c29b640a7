"""CPU-side checks of the device optimizer (virnet_amd/optim.py, csrc/optim.hip): the bindings, the chunk / table planner, the argument
errors (all raised before any device work) and the exchange of state dicts with torch.optim.Adam.  No kernel runs here."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from virnet_amd import _native, optim
from virnet_amd.optim import ClipAdam

NEW_SYMBOLS = ("virnet_optim_plan", "virnet_optim_workspace_bytes", "virnet_optim_grad_norms", "virnet_optim_adam_step", "virnet_optim_scale_grads")


def test_symbols_are_bound_and_the_abi_version_is_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5
    header = open(os.path.join(REPO, "include", "virnet_hip.h")).read()
    assert f"#define VIRNET_OPTIM_CHUNK {optim.CHUNK}\n" in header and f"#define VIRNET_OPTIM_TABLE {optim.TABLE}\n" in header


C_, T_ = optim.CHUNK, optim.TABLE
PLAN_CASES = [
    ([1, 3, 4, 5, 255, C_ - 1, C_, C_ + 1, 2 * C_ + 1], [0, 1, 0, 1, -1, 0, 1, 0, 1]),
    ([7] * (T_ + 1) + [3 * C_], [0] * T_ + [1, -1]),
    ([5] * (2 * T_ + 3), [k % 3 - 1 for k in range(2 * T_ + 3)]),
    ([C_ * 3], [-1]),
    ([2, 9], [2, 0]),                      # (set 1 is empty)
    ([], []),
]


@pytest.mark.parametrize("sizes,sets", PLAN_CASES)
def test_plan_covers_every_element_once_in_set_order(sizes, sets):
    pl = optim.plan(sizes, sets)
    assert pl == optim.plan(sizes, sets)                                     # a pure function of its arguments
    order = pl["order"]
    assert sorted(order) == list(range(len(sizes)))
    keys = [(sets[i] < 0, sets[i]) for i in order]
    assert keys == sorted(keys)                                              # by clip set, tensors in no set last
    for s in set(sets):
        assert [i for i in order if sets[i] == s] == [i for i in range(len(sizes)) if sets[i] == s]      # stable within a set
    # chunks: consecutive ordinals over the ordered list; chunk c of a tensor covers [c * CHUNK, min((c + 1) * CHUNK, size))
    nxt = 0
    for pos, i in enumerate(order):
        assert pl["first_chunk"][pos] == nxt and pl["chunks"][pos] == -(-sizes[i] // C_) >= 1
        covered = np.zeros(sizes[i], dtype=np.int64)
        for c in range(pl["chunks"][pos]):
            lo, hi = c * C_, min((c + 1) * C_, sizes[i])
            assert lo < hi
            covered[lo:hi] += 1
        assert (covered == 1).all()
        nxt += pl["chunks"][pos]
    # tables of at most TABLE tensors, filled in order
    tables = pl["table"]
    assert tables == [pos // T_ for pos in range(len(order))]
    assert all(tables.count(t) <= T_ for t in set(tables))
    # a set's chunks are one contiguous range of ordinals, the sets follow each other
    end = 0
    for s, (first, count) in enumerate(pl["set_range"]):
        mine = [pos for pos, i in enumerate(order) if sets[i] == s]
        assert count == sum(pl["chunks"][pos] for pos in mine)
        if mine:
            assert first == pl["first_chunk"][mine[0]] == end
            assert mine == list(range(mine[0], mine[-1] + 1))
            end = first + count
        else:
            assert (first, count) == (0, 0)


def test_plan_refuses_bad_lists():
    with pytest.raises(RuntimeError, match="elements"):
        optim.plan([4, 0], [0, 0])
    with pytest.raises(RuntimeError, match="elements"):
        optim.plan([1 << 31], [0])
    with pytest.raises(RuntimeError, match="clip set"):
        optim.plan([4], [3], n_sets=2)
    with pytest.raises(ValueError):
        optim.plan([4, 4], [0])
    lib = _native.load()
    numel, sset, out = (C.c_longlong * 2)(4, 4), (C.c_int * 2)(-1, 0), (C.c_int * 2)()
    assert lib.virnet_optim_plan(numel, sset, 2, 1, out, out, out, out) != 0 and b"ordered by set" in lib.virnet_last_error()
    assert lib.virnet_optim_workspace_bytes((C.c_longlong * 2)(C_ + 1, 9), (C.c_int * 2)(0, -1), 2) == 16


def _params(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dtype)) for s in ((3,), (2, 5), (1,))]


def test_argument_errors():
    a, b, c = _params()
    with pytest.raises(ValueError, match="at most one set"):
        ClipAdam([a, b, c], clip=[([a, b], 1.0), ([b], 2.0)])
    with pytest.raises(ValueError, match="amsgrad"):
        ClipAdam([a], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        ClipAdam([a], maximize=True)
    with pytest.raises(TypeError, match="float32"):
        ClipAdam(_params(torch.float16))
    with pytest.raises(TypeError, match="float32"):
        ClipAdam([a], clip=[(_params(torch.float16), 1.0)])
    with pytest.raises(ValueError, match="contiguous"):
        ClipAdam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError, match="max_norm"):
        ClipAdam([a], clip=[([a], -1.0)])
    with pytest.raises(ValueError, match="lr"):
        ClipAdam([a], lr=torch.tensor(1e-3))
    opt = ClipAdam([a, b], clip=[([a], 1.0)])
    with pytest.raises(TypeError, match="float32"):
        opt.add_param_group({"params": _params(torch.float64)})
    with pytest.raises(ValueError, match="amsgrad"):
        opt.add_param_group({"params": [c], "amsgrad": True})


def test_clip_set_member_outside_every_group_is_refused_at_the_step():
    a, b, c = _params()
    opt = ClipAdam([a, b], clip=[([a, c], 1.0)])
    with pytest.raises(ValueError, match="no parameter group"):
        opt.step()
    opt.add_param_group({"params": [c]})                                     # ... and accepted once a group holds it
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()


def test_step_on_cpu_parameters_raises_without_touching_anything():
    a, b, c = _params()
    opt = ClipAdam([a, b, c], lr=1e-2, clip=[([a], 1.0)])
    for p in (a, b, c):
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in (a, b, c)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert all(torch.equal(p, q) for p, q in zip((a, b, c), before)) and len(opt.state) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.clip_grad_norm_([a, b], 1.0)
    with pytest.raises(ValueError, match="2-norm"):
        optim.clip_grad_norm_([a], 1.0, norm_type=1.0)
    with pytest.raises(ValueError, match="error_if_nonfinite"):
        optim.clip_grad_norm_([a], 1.0, error_if_nonfinite=True)


def test_defaults_and_group_keys_are_adams():
    a, b, c = _params()
    ref = torch.optim.Adam([a, b, c], lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    opt = ClipAdam([a, b, c], lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01, clip=[([a, c], 5.0)])
    assert opt.defaults == ref.defaults
    assert opt.state_dict()["param_groups"] == ref.state_dict()["param_groups"]
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 10)              # a scheduler drives param_groups as it drives Adam's
    opt._opt_called = True                                                   # (no step has run here: keep the scheduler's order warning quiet)
    sched.step()
    assert opt.param_groups[0]["lr"] < 3e-4
    dup = copy.deepcopy(opt)                                                 # the clip sets follow the copied parameters
    assert [id(p) for p in dup.clip_sets[0][0]] == [id(dup.param_groups[0]["params"][k]) for k in (0, 2)] and dup.clip_sets[0][1] == 5.0


def _equal_state(x, y):
    assert x["param_groups"] == y["param_groups"]
    assert x["state"].keys() == y["state"].keys()
    for k in x["state"]:
        assert x["state"][k].keys() == y["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in x["state"][k]:
            u, v = x["state"][k][name], y["state"][k][name]
            assert u.dtype == v.dtype and u.device == v.device and u.shape == v.shape and torch.equal(u, v), (k, name)


def test_state_dict_exchange_with_torch_adam():
    params = _params()
    adam = torch.optim.Adam(params, lr=1e-2, betas=(0.85, 0.98), weight_decay=0.1)
    g = torch.Generator().manual_seed(4)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        adam.step()
    sd = adam.state_dict()
    assert float(sd["state"][0]["step"]) == 2.0
    opt = ClipAdam(params, clip=[(params[:2], 1.0)])
    opt.load_state_dict(copy.deepcopy(sd))
    back = opt.state_dict()
    _equal_state(back, sd)
    assert all(st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 for st in opt.state.values())
    fresh = torch.optim.Adam(params)
    fresh.load_state_dict(back)
    _equal_state(fresh.state_dict(), sd)
    fresh.step()                                                             # ... and goes on from step 2
    assert float(fresh.state_dict()["state"][0]["step"]) == 3.0
    # a checkpoint as the training scripts write it
    ckpt = {"optimizer_state_dict": sd}
    again = ClipAdam(params)
    again.load_state_dict(ckpt["optimizer_state_dict"])
    _equal_state(again.state_dict(), sd)
