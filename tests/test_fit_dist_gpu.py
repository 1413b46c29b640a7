"""The fit loops as ranks of a data-parallel job (virnet_amd/fit.py with ``group``; dist.GradientReducer on csrc/gradsync.hip): two ranks on
this box's one GPU over gloo, started ONCE per module as fresh child processes of tests/fit_dist_worker.py, which run every scenario of
tests/fit_dist_cases.py one after another and write their results to a file.  Every test asserts on that file.

The yardstick for "equals one process" is an emulation written out here, not the code under test: two copies of the net, the one-process
batch cut into rows 0-1 and 2-3, each copy's backward on its rows, ``g0 * 0.5 + g1 * 0.5`` in torch (a two-operand sum is order-free, so
gloo's result has the same bits), one ClipAdam step on both.  For the fused denoiser the emulation also does what the ranks do before the
backward: one common power-of-two factor from the MAX of both halves' incoming gradients.  The emulation is run twice; where it repeats
itself bit for bit the two-rank run must equal it bit for bit, otherwise the bars of tests/test_dist_gpu.py:99-100 apply (losses rel 1e-4,
parameter sum rel 1e-5, three steps)."""
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import fit_dist_cases as fc
from virnet_amd import datagen, elbo, fit, schedule, train
from virnet_amd.dist import shard_range
from virnet_amd.optim import ClipAdam

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_LOSS = {"denoise": 4, "sisr": 5}


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    out_dir = str(tmp_path_factory.mktemp("fit_dist"))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "fit_dist_worker.py"), str(r), str(fc.WORLD), str(port), out_dir], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(fc.WORLD)]
    logs, failed = [], False
    for p in procs:
        try:
            logs.append(p.communicate(timeout=60 if failed else 480)[0])
        except subprocess.TimeoutExpired:
            failed = True
            for q in procs:
                q.kill()
            logs.append(p.communicate()[0])
        if p.returncode != 0 and not failed:                   # a dead rank ends its peer; nothing is retried
            failed = True
            for q in procs:
                if q.poll() is None:
                    q.kill()
    assert not failed and all(p.returncode == 0 for p in procs), "\n".join(f"--- rank {r} (exit {p.returncode})\n{log[-3000:]}" for r, (p, log) in enumerate(zip(procs, logs)))
    return [torch.load(os.path.join(out_dir, f"rank{r}.pt"), weights_only=False) for r in range(fc.WORLD)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- the one-process batch and the emulation ---------------------------------------------------------------------------------------------
def _full_batch(name, pool, c, rng, epoch, ii):
    """The whole batch of a step as one process builds it (``rng`` and torch's CPU generator in the loop's state)."""
    task, _, real = fc.SCENARIOS[name]
    b = c["batch_size"]
    if task == "sisr":
        prm = datagen.draw_sisr_params(rng, pool, b, c["hr_size"], c["sf"], c["noise_level"], c["add_jpeg"], c["noise_jpeg"])
        return datagen.sisr_batch(pool, prm, c["hr_size"], c["sf"], c["k_size"], seed=epoch * 1000, downsampler=c["downsampler"],
                                  shift=c["kernel_shift"], base_id=ii * b)
    p = c["patch_size"]
    if real:
        prm, mix = datagen.draw_pair_params(rng, pool, b, p), datagen.draw_mixup_params(b)
        return datagen.real_batch(pool, prm, p, mix, k_size=c["var_window"])
    return datagen.denoise_batch(pool, datagen.draw_denoise_params(rng, pool, b, p), p, seed=epoch, base_id=ii * b)


def _config(name, cfg):
    return fit.read_sisr_config(cfg) if fc.SCENARIOS[name][0] == "sisr" else fit.read_config(cfg)


def emulate(name, epochs=1):
    """-> (rows of half 0, rows of half 1, flat parameters) of the two-rank run as one process computes it."""
    task, mode, real = fc.SCENARIOS[name]
    made = [fc.make(name) for _ in range(2)]
    nets, pool, c = [m[0] for m in made], made[0][1], _config(name, dict(made[0][2], epochs=epochs))
    keys = ("rnet", "snet", "knet") if task == "sisr" else ("rnet", "snet")
    opts = []
    for net in nets:
        named = list(net.named_parameters())
        opts.append(ClipAdam(net.parameters(), lr=c["lr"], clip=[([p for n, p in named if k in n.lower()], c["clip_grad_" + k[0].upper()]) for k in keys]))
    lrs = schedule.cosine(c["lr"], c["lr_min"], epochs) if task == "sisr" else schedule.warmup_cosine(c["lr"], c["lr_min"], epochs, c["warmup_epochs"])
    alpha0 = 0.5 * torch.tensor([c["var_window"] ** 2], dtype=torch.float32).cuda()
    kappa0 = torch.tensor([c["kappa0"]], dtype=torch.float32).cuda() if task == "sisr" else None
    scale = 1000 if task == "sisr" else 1
    rows = [[], []]
    for epoch in range(epochs):
        rng = random.Random(epoch * scale)
        gen = [None, None]
        if task == "sisr" or real:
            torch.manual_seed(epoch * scale)
        if task == "sisr":                                     # rank 1 draws elbo_sisr's samples from its own device stream
            gen[0] = torch.cuda.get_rng_state()
            torch.cuda.manual_seed(epoch * scale + 1)
            gen[1] = torch.cuda.get_rng_state()
        for opt in opts:
            for group in opt.param_groups:
                group["lr"] = lrs[epoch]
        for net in nets:
            net.train()
        for ii in range(c["steps_per_epoch"]):
            batch = _full_batch(name, pool, c, rng, epoch, ii)
            held = []
            for h, (net, opt) in enumerate(zip(nets, opts)):
                a, b = shard_range(c["batch_size"], 2, h)
                part = [None if t is None else t[a:b].contiguous() for t in batch]
                opt.zero_grad()
                if task == "sisr":
                    torch.cuda.set_rng_state(gen[h])
                    im_hr, im_lr, im_blur, kinfo_gt, nlevel = part
                    mu, kinfo_est, sigma_est = net(im_lr, c["sf"])
                    loss, detail = elbo.elbo_sisr(mu=mu, sigma_est=sigma_est, kinfo_est=kinfo_est, im_hr=im_hr, im_lr=im_lr, sigma_prior=nlevel,
                                                  alpha0=alpha0, kinfo_gt=kinfo_gt, kappa0=kappa0, r2=c["r2"], eps2=c["eps2"], sf=c["sf"],
                                                  k_size=c["k_size"], penalty_K=c["penalty_K"], downsampler=c["downsampler"], shift=c["kernel_shift"])
                    loss.backward()
                    gen[h] = torch.cuda.get_rng_state()
                    held.append((loss, list(detail[:4]), None))
                else:
                    im_noisy, im_gt, sigma_gt = part
                    if real:                                   # the variance prior of the rank's rows (per sample: the same bits as the whole batch's rows)
                        sigma_gt = elbo.noise_estimate(im_noisy, im_gt, c["var_window"])
                    mu, sigma = net(im_noisy)
                    loss, lh, kl_g, kl_ig = elbo.elbo_denoising(mu, sigma, im_noisy, im_gt, c["eps2"], alpha0, alpha0 * sigma_gt)
                    if mode == "Input":                        # fused: the backward waits for the common factor
                        held.append((loss, [lh, kl_g, kl_ig], (mu, sigma) + torch.autograd.grad(loss, [mu, sigma])))
                    else:
                        loss.backward()
                        held.append((loss, [lh, kl_g, kl_ig], None))
            if held[0][2] is not None:
                common = torch.maximum(train._amax(*held[0][2][2:]), train._amax(*held[1][2][2:]))      # the ranks' MAX all-reduce
                real_amax = train._amax
                train._amax = lambda *gs: common
                try:
                    for _, _, (mu, sigma, gm, gs) in held:
                        torch.autograd.backward([mu, sigma], [gm, gs])
                finally:
                    train._amax = real_amax
            with torch.no_grad():
                for pa, pb in zip(nets[0].parameters(), nets[1].parameters()):
                    if pa.grad is None and pb.grad is None:
                        continue
                    avg = pa.grad * 0.5 + pb.grad * 0.5
                    pa.grad, pb.grad = avg, avg.clone()
            for h, opt in enumerate(opts):
                opt.step()
                loss, terms, _ = held[h]
                rows[h].append([float(loss.detach())] + [float(t.detach()) for t in terms] + opt.grad_norms.tolist())
    assert _same(fc.flat_params(nets[0]), fc.flat_params(nets[1]))
    return np.asarray(rows[0], dtype=np.float32), np.asarray(rows[1], dtype=np.float32), fc.flat_params(nets[0])


@pytest.fixture(scope="module")
def emulated():
    """name -> (the emulation's result, whether a second run of it gave the same bits)"""
    out = {}
    for name in fc.SCENARIOS:
        first, second = emulate(name), emulate(name)
        repeats = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first[:2], second[:2])) and _same(first[2], second[2])
        print(f"{name}: the emulation {'repeats bit for bit' if repeats else 'does NOT repeat bit for bit: the bars apply'}")
        out[name] = (first, repeats)
    return out


# ---- tests -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.SCENARIOS))
def test_ranks_batches_concatenate_to_the_one_process_batch(ranks, name):
    task, _, real = fc.SCENARIOS[name]
    _, pool, cfg = fc.make(name)
    c = _config(name, cfg)
    scale = 1000 if task == "sisr" else 1
    if task == "sisr" or real:
        torch.manual_seed(0)
    want = _full_batch(name, pool, c, random.Random(0 * scale), 0, 0)
    key = "sisr_batch" if task == "sisr" else ("noise_estimate" if real else "denoise_batch")
    got = [ranks[r][name]["first"][key] for r in range(fc.WORLD)]
    assert len(want) == len(got[0]) == (5 if task == "sisr" else 3)
    for k, w in enumerate(want):
        cat = torch.cat([g[k] for g in got], 0)
        assert cat.shape[0] == 4 and _same(cat, w), (name, k)
        assert not _same(got[0][k], got[1][k])


@pytest.mark.parametrize("name", list(fc.SCENARIOS))
def test_ranks_agree(ranks, name):
    n_loss = N_LOSS[fc.SCENARIOS[name][0]]
    r0, r1 = ranks[0][name], ranks[1][name]
    steps = 6 if name == "sisr" else 3
    assert r0["rows"].shape == r1["rows"].shape == (steps, n_loss + (3 if name == "sisr" else 2))
    assert _same(r0["params"], r1["params"])                                       # parameter bytes
    assert _same(r0["rows"][:, n_loss:], r1["rows"][:, n_loss:])                   # the norms of the AVERAGED gradients
    assert bool((r0["rows"][:, 0] != r1["rows"][:, 0]).all())                      # each rank logs its own shard's loss
    assert bool(torch.isfinite(r0["rows"]).all()) and bool(torch.isfinite(r1["rows"]).all())
    assert (r0["world"], r0["rank"], r1["world"], r1["rank"]) == (2, 0, 2, 1)
    assert r0["lines"] and not r1["lines"]                                         # only rank 0 logs
    assert not r1["checkpoints"] and len(r0["checkpoints"]) == (2 if name == "sisr" else 0)
    assert not r0["leftover"] and not r1["leftover"]
    # exactly one averaging per step, by the route the backward took: the fused Function feeds the reducer, the per-conv route does not
    fused = fc.SCENARIOS[name][1] == "Input"
    assert r0["routes"] == r1["routes"] == ({"finish": steps, "reduce_grads": 0} if fused else {"finish": 0, "reduce_grads": steps})


@pytest.mark.parametrize("name", list(fc.SCENARIOS))
def test_two_ranks_equal_the_emulation(ranks, emulated, name):
    (rows0, rows1, params), repeats = emulated[name]
    got = [ranks[r][name] for r in range(2)]
    if name == "sisr":                                                             # (the ranks ran two epochs for the resume test)
        ckpt = torch.load(got[0]["checkpoints"][0], map_location="cpu")
        got_params = torch.cat([ckpt["model_state_dict"][k].reshape(-1) for k, _ in fc.sr_net().named_parameters()])
    else:
        got_params = got[0]["params"]
    got_rows = [g["rows"][:3].numpy() for g in got]
    print(f"{name}: exact={repeats}; rank-0 losses {got_rows[0][:, 0]} emulated {rows0[:, 0]}; psum {float(got_params.double().sum())!r} "
          f"emulated {float(params.double().sum())!r}")
    if repeats:
        assert np.array_equal(got_rows[0].view(np.uint32), rows0.view(np.uint32)) and np.array_equal(got_rows[1].view(np.uint32), rows1.view(np.uint32))
        assert _same(got_params, params)
    else:
        n_loss = N_LOSS[fc.SCENARIOS[name][0]]
        assert got_rows[0][:, 0] == pytest.approx(rows0[:, 0], rel=1e-4) and got_rows[1][:, 0] == pytest.approx(rows1[:, 0], rel=1e-4)
        assert float(got_params.double().sum()) == pytest.approx(float(params.double().sum()), rel=1e-5)
        assert got_rows[0].shape[1] > n_loss


def test_sisr_resume_across_ranks(ranks, emulated):
    """one epoch + resume + one epoch == two epochs, both on two ranks; the rule for bit-equal versus the bars is the SISR step's"""
    repeats = emulated["sisr"][1]
    for r in range(2):
        straight, resumed = ranks[r]["sisr"], ranks[r]["sisr_resume"]
        assert resumed["epoch_start"] == 1 and resumed["rows"].shape == (3, 8)
        if repeats:
            assert _same(resumed["rows"], straight["rows"][3:]) and _same(resumed["params"], straight["params"])
        else:
            assert resumed["rows"][:, 0].numpy() == pytest.approx(straight["rows"][3:, 0].numpy(), rel=1e-4)
            assert float(resumed["params"].double().sum()) == pytest.approx(float(straight["params"].double().sum()), rel=1e-5)


def test_batch_the_world_does_not_divide_is_refused(ranks):
    for r in range(2):
        msg = ranks[r]["indivisible"]
        assert msg is not None and "3" in msg and "world size 2" in msg


def test_world_one_is_untouched():
    """``group=None`` and no process group: the loop a user writes by hand on the whole batch (what tests/test_fit_gpu.py pins the loop
    to), bit for bit in rows and parameters; no reducer is attached, ``world`` is 1."""
    assert not torch.distributed.is_initialized()
    net, pool, cfg = fc.make("syn_fused")
    lines = []
    out = fit.fit_denoising(net, pool, cfg, log=lines.append)
    assert (out["world"], out["rank"]) == (1, 0) and not hasattr(net, "_grad_reducer") and len(lines) == 5
    ref, _, _ = fc.make("syn_fused")
    c = fit.read_config(cfg)
    named = list(ref.named_parameters())
    opt = ClipAdam(ref.parameters(), lr=c["lr"], clip=[([p for n, p in named if "rnet" in n.lower()], c["clip_grad_R"]),
                                                      ([p for n, p in named if "snet" in n.lower()], c["clip_grad_S"])])
    for group in opt.param_groups:
        group["lr"] = schedule.warmup_cosine(c["lr"], c["lr_min"], 1, 0)[0]
    alpha0 = 0.5 * torch.tensor([49.0], dtype=torch.float32).cuda()
    rng, rows = random.Random(0), []
    ref.train()
    for ii in range(3):
        im_noisy, im_gt, sigma_gt = _full_batch("syn_fused", pool, c, rng, 0, ii)
        opt.zero_grad()
        mu, sigma = ref(im_noisy)
        loss, lh, kl_g, kl_ig = elbo.elbo_denoising(mu, sigma, im_noisy, im_gt, c["eps2"], alpha0, alpha0 * sigma_gt)
        loss.backward()
        opt.step()
        rows.append([float(loss.detach()), float(lh), float(kl_g), float(kl_ig)] + opt.grad_norms.tolist())
    assert np.array_equal(out["rows"].view(np.uint32), np.asarray(rows, dtype=np.float32).view(np.uint32))
    assert _same(fc.flat_params(net), fc.flat_params(ref))
