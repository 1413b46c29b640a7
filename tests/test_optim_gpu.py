"""virnet_amd.optim on the device against fp64 and against the route the reference project calls (tests/optim_cases.py holds the tensor
set, the references and the bound rule).

Every bound test prints the largest error of both routes per state, in fp32 ulps of the tensor's largest magnitude (run with -s); the
figures of an MI355X run are in profiles/optim_device.md."""
import copy
import io
import math

import numpy as np
import pytest
import torch

import optim_cases as oc
from virnet_amd.optim import ClipAdam
from optim_cases import I_NOGRAD, I_NOSET, MAX_NORMS

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _norm_within_one_ulp(got, want64):
    return abs(float(got) - want64) <= oc.ulp(want64)


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_single_step_against_fp64(t):
    ref, tor = oc.fp64_run(t, [0]), oc.torch_run(t, [0])
    dev = oc.device_run(t, [0])
    oc.check_bound(dev, tor, ref, f"single step t={t}")
    norms, coefs = dev["norms"][0], dev["coefs"][0]
    assert norms.dtype == torch.float32 and norms.shape == (2,) and coefs.shape == (2,)
    for s in (0, 1):
        print(f"set {s}: norm device {float(norms[s])!r} torch {tor['norms'][0][s]!r} fp64 {ref['norms'][0][s]!r}")
        assert _norm_within_one_ulp(norms[s], ref["norms"][0][s])
    assert ref["norms"][0][0] > MAX_NORMS[0] and ref["norms"][0][1] < MAX_NORMS[1]          # one set clipped, one not
    assert float(coefs[1]) == 1.0
    assert abs(float(coefs[0]) - ref["coefs"][0][0]) <= 2 * oc.ulp(ref["coefs"][0][0])       # the norm's rounding, then the quotient's
    # per-parameter step counts
    for i, p in enumerate(dev["params"]):
        st = dev["opt"].state.get(p)
        if i == I_NOGRAD:
            assert (st is None) if t == 1 else float(st["step"]) == t - 1
        else:
            assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == t


def test_trajectory_of_three_steps():
    seeds = [0, 1, 2]
    for t in (1, 1000):
        oc.check_bound(oc.device_run(t, seeds), oc.torch_run(t, seeds), oc.fp64_run(t, seeds), f"three steps from t={t}")


def test_learning_rate_is_read_at_every_step():
    seeds, lrs = [0, 1], [1e-3, 5e-2]
    ref, tor, dev = oc.fp64_run(1, seeds, lrs), oc.torch_run(1, seeds, lrs), oc.device_run(1, seeds, lrs)
    oc.check_bound(dev, tor, ref, "lr 1e-3 then 5e-2")
    stale = oc.fp64_run(1, seeds)                              # had the second step kept the first lr, p would be far from the reference
    assert max(float((a - b).abs().max()) for a, b in zip(stale["p"], ref["p"])) > 1e-2


def test_weight_decay_follows_the_l2_form():
    ref, tor = oc.fp64_run(2, [0], weight_decay=0.05), oc.torch_run(2, [0], weight_decay=0.05)
    oc.check_bound(oc.device_run(2, [0], weight_decay=0.05), tor, ref, "weight_decay 0.05")


def test_skips_and_versions():
    params, buf = oc.make_params(1000, "cuda")
    opt = oc.clip_adam(params)
    oc.load_start(opt, params, 1000)
    oc.set_grads(params, 0)
    before = [p.detach().clone() for p in params]
    st = opt.state[params[I_NOGRAD]]
    kept = (st["step"].clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    versions = [p._version for p in params]
    edge = (buf[0].clone(), buf[1 + oc.VIEW_LEN:].clone())
    opt.step()
    assert _same_bits(params[I_NOGRAD], before[I_NOGRAD]) and params[I_NOGRAD]._version == versions[I_NOGRAD]
    assert torch.equal(st["step"], kept[0]) and _same_bits(st["exp_avg"], kept[1]) and _same_bits(st["exp_avg_sq"], kept[2])
    for i, p in enumerate(params):
        if i != I_NOGRAD:
            assert p._version > versions[i], i
            assert not torch.equal(p, before[i]), i
    assert _same_bits(buf[0], edge[0]) and _same_bits(buf[1 + oc.VIEW_LEN:], edge[1])      # the view's neighbours in its buffer
    # the parameter in no set is stepped with its gradient as it is: bitwise what a ClipAdam without clip sets computes
    lone = torch.nn.Parameter(before[I_NOSET].clone())
    plain = ClipAdam([lone], lr=oc.LR, betas=oc.BETAS, eps=oc.EPS)
    _, m0, v0, step, _ = oc.start(1000)
    plain.state[lone] = {"step": torch.tensor(step), "exp_avg": m0[I_NOSET].cuda(), "exp_avg_sq": v0[I_NOSET].cuda()}
    lone.grad = params[I_NOSET].grad.clone()
    plain.step()
    assert plain.grad_norms is None and _same_bits(lone, params[I_NOSET])


@pytest.mark.parametrize("write_back", [False, True])
def test_gradient_write_back(write_back):
    params, _ = oc.make_params(1, "cuda")
    opt = oc.clip_adam(params, write_back_grads=write_back)
    oc.set_grads(params, 0)
    g0 = [None if p.grad is None else p.grad.clone() for p in params]
    opt.step()
    coefs = opt.clip_coefs
    for i, p in enumerate(params):
        if g0[i] is None:
            assert p.grad is None
        elif write_back and oc.set_of(i) >= 0:
            assert _same_bits(p.grad, g0[i] * coefs[oc.set_of(i)]), i
        else:
            assert _same_bits(p.grad, g0[i]), i


def test_non_contiguous_gradient_goes_through_a_contiguous_copy():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(6, 10, generator=g)
    gr = torch.randn(10, 6, generator=g) * 30
    outs = []
    for strided in (False, True):
        p = torch.nn.Parameter(w.cuda())
        opt = ClipAdam([p], lr=1e-2, clip=[([p], 1.0)], write_back_grads=True)
        p.grad = gr.cuda().t() if strided else gr.t().contiguous().cuda()
        assert p.grad.is_contiguous() != strided
        opt.step()
        outs.append((p.detach().clone(), p.grad.clone(), opt.grad_norms.clone()))
    assert all(_same_bits(a, b) for a, b in zip(*outs))


def test_clip_grad_norm_against_torch_cpu():
    from virnet_amd.optim import clip_grad_norm_
    dev_params, _ = oc.make_params(1, "cuda")
    cpu_params, _ = oc.make_params(1, "cpu")
    for s in (0, 1):
        oc.set_grads(dev_params, 3)
        oc.set_grads(cpu_params, 3)
        g0 = [None if p.grad is None else p.grad.double() for p in cpu_params]
        want64 = math.sqrt(sum(float((g ** 2).sum()) for i, g in enumerate(g0) if g is not None and oc.set_of(i) == s))
        got = clip_grad_norm_(oc.members(dev_params, s), MAX_NORMS[s])
        want = torch.nn.utils.clip_grad_norm_(oc.members(cpu_params, s), MAX_NORMS[s])
        assert got.is_cuda and got.dtype == torch.float32 and got.dim() == 0
        print(f"set {s}: norm device {float(got)!r} torch {float(want)!r} fp64 {want64!r}")
        assert _norm_within_one_ulp(got, want64)
        # the coefficient as the kernels define it: fp32 arithmetic on the fp32 rounding of the fp64 norm
        norm32 = np.float32(want64)
        coef = float(min(np.float32(MAX_NORMS[s]) / (norm32 + np.float32(1e-6)), np.float32(1.0)))
        for i, (p, q) in enumerate(zip(dev_params, cpu_params)):
            if g0[i] is None:
                assert p.grad is None
            elif oc.set_of(i) != s:
                assert _same_bits(p.grad, oc.grads(3)[i])                               # other sets' gradients are not touched
            else:
                exact = g0[i] * coef                                                    # (fp64: the product of two fp32 values is exact)
                err = (p.grad.cpu().double() - exact).abs()
                one_ulp = torch.from_numpy(np.spacing(exact.abs().float().numpy())).double()
                assert bool((err <= one_ulp).all()), (s, i, float((err / one_ulp).max()))
                # torch's own norm is an fp32 sum (a few ulps off, printed above) and its coefficient reciprocal * max_norm: 1e-6 relative
                assert torch.allclose(p.grad.cpu(), q.grad, rtol=1e-6, atol=0.0), (s, i)
                if coef == 1.0:
                    assert _same_bits(p.grad, q.grad)
    assert float(clip_grad_norm_([], 1.0)) == 0.0
    lone = torch.nn.Parameter(torch.ones(3, device="cuda"))
    assert float(clip_grad_norm_(lone, 1.0)) == 0.0 and lone.grad is None                 # no gradient anywhere: torch's answer


def test_non_finite_gradient_gives_torchs_pattern():
    def poison(params):
        oc.set_grads(params, 0)
        params[4].grad[17] = float("inf")                                                  # a member of set 0

    cpu, _ = oc.make_params(1, "cpu")
    adam = torch.optim.Adam(cpu, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS, foreach=False)
    poison(cpu)
    for s in (0, 1):
        torch.nn.utils.clip_grad_norm_(oc.members(cpu, s), MAX_NORMS[s])
    adam.step()
    dev, _ = oc.make_params(1, "cuda")
    opt = oc.clip_adam(dev)
    poison(dev)
    opt.step()
    assert math.isinf(float(opt.grad_norms[0])) and float(opt.clip_coefs[0]) == 0.0
    start = oc.start(1)[0]
    n_nan = 0
    for i, (p, q) in enumerate(zip(dev, cpu)):
        p = p.detach().cpu()
        assert torch.equal(torch.isnan(p), torch.isnan(q.detach())), i
        assert torch.equal(p == start[i], q.detach() == start[i]), i                       # a zero gradient leaves p where it was
        n_nan += int(torch.isnan(p).sum())
    assert n_nan == 1


def test_bitwise_reproducible_also_when_the_gradients_move():
    runs = []
    for fresh in (False, False, True):
        params, _ = oc.make_params(2, "cuda")
        opt = oc.clip_adam(params)
        oc.load_start(opt, params, 2)
        norms, ballast = [], []
        for seed in (0, 1, 2):
            if fresh:
                ballast.append(torch.empty(1000 + 3 * 17 * len(ballast), device="cuda"))      # the allocator hands out other addresses
                old = [p.grad for p in params]
                oc.set_grads(params, seed)
                ballast += old
            elif params[0].grad is None:
                oc.set_grads(params, seed)
            else:
                for p, g in zip(params, oc.grads(seed)):
                    if g is not None:
                        p.grad.copy_(g)
            opt.step()
            norms.append(opt.grad_norms.clone())
        out = oc.state_lists(opt, params)
        runs.append(out["p"] + out["m"] + out["v"] + norms)
    for other in runs[1:]:
        assert all(_same_bits(a, b) for a, b in zip(runs[0], other))


def test_handover_from_and_to_torch_adam():
    """two steps in one optimizer on CUDA, then its state_dict() goes into BOTH kinds, each over its own copy of the parameters, and both
    run two more steps.  ClipAdam's end is held to the trajectory bound against fp64 from the state that was handed over, and the two ends
    agree with each other within that same bound (the distance over the bound is printed)."""

    def steps(opt, params, seeds):
        for seed in seeds:
            oc.set_grads(params, seed)
            if isinstance(opt, torch.optim.Adam):
                for s in (0, 1):
                    torch.nn.utils.clip_grad_norm_(oc.members(params, s), MAX_NORMS[s])
            opt.step()

    def adam_over(params):
        return torch.optim.Adam(params, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS)

    for first in (adam_over, oc.clip_adam):
        params, _ = oc.make_params(1, "cuda")
        giver = first(params)
        steps(giver, params, [0, 1])
        mid, sd = oc.snapshot(giver, params), giver.state_dict()
        assert mid[3][0] == 2.0 and mid[3][oc.I_NOGRAD] == 0.0
        ends = []
        for kind in (oc.clip_adam, adam_over):
            mine, _ = oc.make_params(mid, "cuda")
            taker = kind(mine)
            taker.load_state_dict(copy.deepcopy(sd))
            steps(taker, mine, [2, 3])
            assert all(float(st["step"]) == 4.0 and st["step"].device.type == "cpu" for st in taker.state.values())
            ends.append(oc.state_lists(taker, mine))
        ref, tor = oc.fp64_run(mid, [2, 3]), oc.torch_run(mid, [2, 3])
        label = f"two steps after two of {'torch' if first is adam_over else 'ClipAdam'}"
        oc.check_bound(ends[0], tor, ref, label)
        apart, far = 0.0, []
        for what in ("p", "m", "v"):
            for i, (a, b) in enumerate(zip(ends[0][what], ends[1][what])):
                if a is None:
                    continue
                e_tor = float((tor[what][i].double() - ref[what][i]).abs().max())
                bound = max(2.0 * e_tor, oc.ulp(float(ref[what][i].abs().max())))
                d = float((a.double() - b.double()).abs().max())
                apart = max(apart, d / bound)
                if not d <= bound:
                    far.append((what, i, d, bound))
        print(f"optim handover {label}: ClipAdam and torch-CUDA ends are at most {apart:.3f} of the trajectory bound apart")
        assert not far, (label, far)
    dup = copy.deepcopy(giver)                                                          # (the last giver is a ClipAdam after two steps)
    assert isinstance(dup, ClipAdam) and dup.clip_sets[0][1] == MAX_NORMS[0] and len(dup.state) == len(giver.state)
    assert all(_same_bits(a["exp_avg"], b["exp_avg"]) and a["exp_avg"].data_ptr() != b["exp_avg"].data_ptr()
               for a, b in zip(dup.state.values(), giver.state.values()))
    oc.set_grads(dup.param_groups[0]["params"], 0)
    dup.step()                                                                          # the copy steps its own parameters
    assert float(next(iter(dup.state.values()))["step"]) == 3.0 and float(next(iter(giver.state.values()))["step"]) == 2.0
    buffer = io.BytesIO()
    torch.save(giver.state_dict(), buffer)
    assert buffer.tell() > 0


def test_network_training_follows_the_step():
    """four ClipAdam steps on the network of test_optimizer_step_and_repack; afterwards the module's own forwards (packed weights, composed
    tail, graphs) equal those of a fresh module loaded from its state_dict, bit for bit"""
    from virnet_amd.networks import VIRAttResUNet
    from virnet_amd.utils.synth import synth_images, synth_state_dict
    cfg = dict(sigma_chn=1, n_feat=[64, 96], dep_S=3, n_resblocks=1)
    net = VIRAttResUNet(3, **cfg).cuda()
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=6))
    p_r = [p for n_, p in net.named_parameters() if "rnet" in n_.lower()]
    p_s = [p for n_, p in net.named_parameters() if "snet" in n_.lower()]
    opt = ClipAdam(net.parameters(), lr=1e-3, clip=[(p_r, 1e3), (p_s, 1e2)])
    x = synth_images(2, 3, 16, 32).cuda()
    gt = synth_images(2, 3, 16, 32, seed=9).cuda()
    losses = []
    for _ in range(4):
        opt.zero_grad()
        mu, sigma = net(x)
        loss = ((mu - gt) ** 2).mean() + 0.01 * (sigma.log() ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses
    assert opt.grad_norms.shape == (2,) and bool(torch.isfinite(opt.grad_norms).all()) and bool((opt.grad_norms > 0).all())
    fresh = VIRAttResUNet(3, **cfg).cuda()
    fresh.load_state_dict(net.state_dict())
    for mode in ("eval", "train"):
        getattr(net, mode)()
        getattr(fresh, mode)()
        with torch.no_grad():
            a, b = net(x), fresh(x)
        assert all(_same_bits(u, v) for u, v in zip(a, b)), mode
