"""The device training loop on the GPU (virnet_amd/fit.py, trainlog.py, datagen.SimulateTestSet; csrc/trainlog.hip, csrc/datagen.hip): the
validation kernel against its numpy definition (which tests/test_fit_host.py pins to the reference's ``SimulateTest``) bit for bit and under
the software red zone, the step log against the Python accumulation it replaces, ``fit_denoising`` against the loop a user writes from the
README with the same seeds -- parameters and logged values bit for bit, synthetic and real noise -- the bitwise resume, the absence of
host synchronisation between two log reads, and the validation stage against the host metrics."""
import random

import numpy as np
import pytest
import torch

import datagen_cases as dc
from redzone import guarded
from virnet_amd import datagen, elbo, fit, schedule, trainlog
from virnet_amd import eval as veval
from virnet_amd.networks import VIRAttResUNet
from virnet_amd.optim import ClipAdam
from virnet_amd.utils.synth import synth_state_dict

pytestmark = pytest.mark.gpu

SIM_SHAPES = [(1, 1), (7, 300), (300, 7), (33, 65), (56, 40)]
NET = dict(sigma_chn=1, n_feat=[32, 64], dep_S=3, n_resblocks=1)
CFG = dict(batch_size=4, patch_size=32, epochs=2, warmup_epochs=1, lr=1e-4, lr_min=1e-6, print_freq=2, clip_grad_R=1e3, clip_grad_S=1e2,
           var_window=7, eps2=1e-6, steps_per_epoch=3)


# ---- the validation kernel -------------------------------------------------------------------------------------------------------------------
def _sim_images():
    """two images per shape of SIM_SHAPES (image 2 s and 2 s + 1), then one that makes h_max = 310, w_max = 320: larger than any of them"""
    g = np.random.default_rng(7)
    ims = []
    for h, w in SIM_SHAPES:
        ims += [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    return ims + [g.integers(0, 256, (310, 320, 3), dtype=np.uint8)]


@pytest.fixture(scope="module")
def sim_set():
    ims = _sim_images()
    vs = datagen.SimulateTestSet(datagen.ImagePool(ims, "cuda"))
    assert (vs.h_max, vs.w_max) == (310, 320)
    return ims, vs


@pytest.mark.parametrize("s", range(len(SIM_SHAPES)), ids=[str(s) for s in SIM_SHAPES])
def test_validation_kernel_is_the_definition_bit_for_bit(sim_set, s):
    ims, vs = sim_set
    for idx in ([2 * s], [2 * s + 1, 2 * s, 2 * s + 1]):          # n = 1 and 3, an index that repeats
        noisy, gt = vs.batch(idx)
        want_noisy, want_gt = datagen.simulate_test_np(ims, idx, vs.noise_np, vs.sigma_map_np)
        assert noisy.shape == gt.shape == (len(idx), 3) + SIM_SHAPES[s] and noisy.dtype == gt.dtype == torch.float32
        assert dc.same_bits(noisy, want_noisy) and dc.same_bits(gt, want_gt)
    assert torch.equal(vs.batch([2 * s])[0], vs.batch([2 * s, 2 * s])[0][1:])          # an image does not depend on its place in the batch


@pytest.mark.parametrize("s", range(len(SIM_SHAPES)), ids=[str(s) for s in SIM_SHAPES])
def test_validation_kernel_stays_inside_its_buffers(s, monkeypatch):
    """Pool, table, noise, sigma map and both index tables enter through ``g.input``; the image indices and the outputs come from the
    package's own ``torch.empty`` inside the guard.  A stray read of the uint8 pool cannot show up as NaN, so values are compared too."""
    ims = _sim_images()
    idx = [2 * s + 1, 2 * s, 2 * s + 1]
    with guarded() as g:
        pool = datagen.ImagePool(ims, "cuda")
        pool.data, pool.table = g.input(pool.data), g.input(pool.table)
        vs = datagen.SimulateTestSet(pool)
        vs.noise, vs.sigma_map = g.input(vs.noise), g.input(vs.sigma_map)
        cached = datagen._device_nearest
        monkeypatch.setattr(datagen, "_device_nearest", lambda size, device: g.input(cached(size, device)))
        out = vs.batch(idx)
        g.check(out)
        want = datagen.simulate_test_np(ims, idx, vs.noise_np, vs.sigma_map_np)
        assert dc.same_bits(out[0], want[0]) and dc.same_bits(out[1], want[1])


# ---- the step log ----------------------------------------------------------------------------------------------------------------------------
def test_step_log_rows_and_sums_are_bitwise_the_python_loop():
    names, num_iter = ["Loss", "lh", "KLG", "KLIG", "GNorm_R", "GNorm_S"], 37
    g = np.random.default_rng(3)
    vals = (g.standard_normal((40, 6)) * np.asarray([1e3, 1.0, 1e-3, 10.0, 1e4, 1e-2])).astype(np.float32)
    dev = torch.from_numpy(vals).cuda()
    log = trainlog.StepLog(names, capacity=8, num_iter=num_iter)
    acc = [0.0] * 6
    got_rows = []
    reads = {0, 3, 4, 11, 19, 20, 27, 33, 39}          # irregular, never more than 8 steps apart
    for step in range(40):
        row = dev[step]
        log.push(row[0], row[1], row[2], row[3], row[4:6])          # four 0-dim tensors and a 1-D one, as the loop pushes them
        for t in range(6):
            acc[t] += float(vals[step, t]) / num_iter                # the reference's `+= x.item() / num_iter`
        if step in reads:
            rows, sums = log.read()
            got_rows.append(rows)
            assert sums.dtype == np.float64 and sums.tolist() == acc, step
    got = np.concatenate(got_rows)
    assert got.dtype == np.float32 and got.shape == (40, 6) and np.array_equal(got.view(np.uint32), vals.view(np.uint32))
    assert log.read()[0].shape == (0, 6)
    # a push that would overwrite an unread slot is refused; a read makes room again
    for step in range(8):
        log.push(dev[step, 0], dev[step, 1], dev[step, 2], dev[step, 3], dev[step, 4:6])
    with pytest.raises(RuntimeError, match="overwrite slot 0"):
        log.push(dev[8, 0], dev[8, 1], dev[8, 2], dev[8, 3], dev[8, 4:6])
    rows, _ = log.read()
    assert np.array_equal(rows.view(np.uint32), vals[:8].view(np.uint32))
    log.reset()
    log.push(dev[8, 0], dev[8, 1], dev[8, 2], dev[8, 3], dev[8, 4:6])
    rows, sums = log.read()
    assert np.array_equal(rows.view(np.uint32), vals[8:9].view(np.uint32)) and sums.tolist() == [float(v) / num_iter for v in vals[8]]
    with pytest.raises(RuntimeError, match=r"argument 4 \('GNorm_R', 'GNorm_S'\) is on cpu"):
        log.push(dev[0, 0], dev[0, 1], dev[0, 2], dev[0, 3], torch.zeros(2))


# ---- the loop --------------------------------------------------------------------------------------------------------------------------------
def _net(sigma_chn=1):
    cfg = dict(NET, sigma_chn=sigma_chn)
    net = VIRAttResUNet(3, **cfg)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=11))
    return net.cuda()


def _pool_images(seed):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (48, 48, 3), dtype=np.uint8) for _ in range(4)]


def _val_images():
    g = np.random.default_rng(5)
    return [g.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((24, 20), (20, 24), (24, 20))]


def readme_loop(net, pool, cfg, real, epochs=None):
    """The loop a user writes from the README's lines, with the reference's per-step host reads (train_denoising_syn.py:169-198)."""
    named = list(net.named_parameters())
    params_r, params_s = [p for n, p in named if "rnet" in n.lower()], [p for n, p in named if "snet" in n.lower()]
    opt = ClipAdam(net.parameters(), lr=cfg["lr"], clip=[(params_r, cfg["clip_grad_R"]), (params_s, cfg["clip_grad_S"])])
    lrs = schedule.warmup_cosine(cfg["lr"], cfg["lr_min"], cfg["epochs"], cfg["warmup_epochs"])
    alpha0 = 0.5 * torch.tensor([cfg["var_window"] ** 2], dtype=torch.float32).cuda()
    b, p, num_iter = cfg["batch_size"], cfg["patch_size"], cfg["steps_per_epoch"]
    rows, means = [], []
    for epoch in range(cfg["epochs"] if epochs is None else epochs):
        rng = random.Random(epoch)
        if real:
            torch.manual_seed(epoch)
        for group in opt.param_groups:
            group["lr"] = lrs[epoch]
        net.train()
        per_epoch = {x: 0 for x in ("Loss", "lh", "KLG", "KLIG")}
        for step in range(num_iter):
            if real:
                prm, mix = datagen.draw_pair_params(rng, pool, b, p), datagen.draw_mixup_params(b)
                im_noisy, im_gt, sigma_gt = datagen.real_batch(pool, prm, p, mix, k_size=cfg["var_window"])
            else:
                im_noisy, im_gt, sigma_gt = datagen.denoise_batch(pool, datagen.draw_denoise_params(rng, pool, b, p), p, epoch, base_id=step * b)
            beta0 = alpha0 * sigma_gt
            opt.zero_grad()
            mu, sigma = net(im_noisy)
            loss, lh, kl_g, kl_ig = elbo.elbo_denoising(mu, sigma, im_noisy, im_gt, cfg["eps2"], alpha0, beta0)
            loss.backward()
            opt.step()
            for key, v in zip(per_epoch, (loss, lh, kl_g, kl_ig)):
                per_epoch[key] += v.item() / num_iter
            rows.append([loss.item(), lh.item(), kl_g.item(), kl_ig.item()] + opt.grad_norms.tolist())
        means.append(per_epoch)
    return np.asarray(rows, dtype=np.float32), means, opt


def _same_state(net_a, net_b):
    return all(torch.equal(a, b) for a, b in zip(net_a.state_dict().values(), net_b.state_dict().values()))


def _same_adam(opt_a, opt_b):
    sa, sb = opt_a.state_dict()["state"], opt_b.state_dict()["state"]
    return sa.keys() == sb.keys() and len(sa) > 0 and all(
        float(sa[k]["step"]) == float(sb[k]["step"]) and torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"])
        and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"]) for k in sa)


@pytest.fixture(scope="module")
def syn_run(tmp_path_factory):
    """fit_denoising for 2 epochs x 3 steps with validation and checkpoints: shared (read-only) by the tests below"""
    save_dir = tmp_path_factory.mktemp("fit_syn")
    pool = datagen.ImagePool(_pool_images(1), "cuda")
    val = datagen.SimulateTestSet(datagen.ImagePool(_val_images(), "cuda"))
    net = _net()
    lines = []
    out = fit.fit_denoising(net, pool, CFG, val=val, save_dir=save_dir, log=lines.append)
    return dict(net=net, pool=pool, val=val, out=out, lines=lines, save_dir=save_dir)


def test_fit_is_the_readme_loop_bit_for_bit(syn_run):
    out = syn_run["out"]
    ref_net = _net()
    rows, means, opt = readme_loop(ref_net, syn_run["pool"], CFG, real=False)
    assert out["rows"].shape == (6, 6) and np.array_equal(out["rows"].view(np.uint32), rows.view(np.uint32))
    assert out["train"] == means                                                   # the epoch means: the same Python doubles
    assert _same_state(syn_run["net"], ref_net)
    print("Adam state also bitwise:", _same_adam(out["optimizer"], opt))
    assert out["lr"] == schedule.warmup_cosine(1e-4, 1e-6, 2, 1) and out["epoch_start"] == 0
    # the reference's lines, the whole transcript: per epoch steps 1 and 2 of 3 are printed (ii == 0, print_freq 2), then the epoch line, a
    # rule, the test line (the mean of the epoch's per-image values), a rule and the time line (its figure is not compared)
    lines, took, want = syn_run["lines"], "This epoch take time ", []
    for e in range(2):
        want += [fit.train_line(e, 2, ii, 3, rows[3 * e + ii], 1e3, 1e2, out["lr"][e]) for ii in (0, 1)]
        want += [fit.epoch_line([means[e][k] for k in ("Loss", "lh", "KLG", "KLIG")]), "-" * 150]
        psnrs, ssims = out["val_images"][e]
        want += [f"test: PSNR={float(np.mean(psnrs)):4.2f}, SSIM={float(np.mean(ssims)):5.4f}", "-" * 90, took]
    assert [line[:len(took)] if line.startswith(took) else line for line in lines] == want
    assert lines[0].startswith("[Epoch: 1/2 ] train:00001/00003, lh=") and lines[7].startswith("[Epoch: 2/2 ] train:00001/00003, lh=")
    assert all(float(lines[k][len(took):]) >= 0.0 for k in (6, 13))
    assert out["step"] == 4 and np.isfinite(out["rows"]).all() and not np.array_equal(rows[0], rows[3])


def test_fit_real_is_the_readme_loop_bit_for_bit():
    pool = datagen.ImagePool.paired(_pool_images(2), _pool_images(3), "cuda")
    cfg = dict(CFG, clip_grad_R=5e2)
    net, ref_net = _net(3), _net(3)
    g = np.random.default_rng(8)
    blocks = [[g.integers(0, 256, (24, 24, 3), dtype=np.uint8) for _ in range(3)] for _ in range(2)]
    with pytest.raises(TypeError, match="paired pool"):
        fit.fit_denoising(net, pool, cfg, real=True, val=datagen.ImagePool(blocks[0], "cuda"), log=lambda s: None)
    out = fit.fit_denoising(net, pool, cfg, real=True, val=datagen.ImagePool.paired(blocks[0], blocks[1], "cuda"), log=lambda s: None)
    # the test stage on the paired blocks (train_denoising_real.py:214-247): img_as_float32 inputs, host metrics on the same outputs
    net.eval()
    psnrs, ssims = [], []
    with torch.no_grad():
        for noisy, gt in zip(*blocks):
            mu = net(torch.from_numpy(np.ascontiguousarray(veval.img_as_float32(noisy).transpose(2, 0, 1)[None])).cuda())[0]
            den = veval.img_as_ubyte(np.clip(mu[0].cpu().numpy().transpose(1, 2, 0), 0.0, 1.0))
            psnrs.append(veval.calculate_psnr(den, gt))
            ssims.append(veval.calculate_ssim(den, gt))
    assert out["val_images"][-1][0] == psnrs and max(abs(a - b) for a, b in zip(out["val_images"][-1][1], ssims)) <= 1e-10
    assert out["psnr"][-1] == float(np.mean(psnrs)) and len(out["psnr"]) == 2
    rows, means, opt = readme_loop(ref_net, pool, cfg, real=True)
    assert out["rows"].shape == (6, 6) and np.array_equal(out["rows"].view(np.uint32), rows.view(np.uint32))
    assert out["train"] == means and _same_state(net, ref_net)
    print("Adam state also bitwise:", _same_adam(out["optimizer"], opt))
    assert np.isfinite(out["rows"]).all()


def test_a_checkpoint_restores_parameters_and_adam_state_bit_for_bit(syn_run):
    """What a resume starts from: loading model_2.pth into a zeroed network and a fresh optimizer gives the straight run's final
    parameters, Adam moments and step counts, bit for bit, and the reference's four keys are there."""
    path = syn_run["out"]["checkpoints"][1]
    ckpt = torch.load(path, map_location="cpu")
    assert set(ckpt) == {"epoch", "step", "step_img", "model_state_dict", "optimizer_state_dict"} and ckpt["epoch"] == 2 and ckpt["step"] == 5
    net = _net()
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
    opt = ClipAdam(net.parameters(), lr=1.0)
    assert fit.load_checkpoint(path, net, opt, map_location="cuda")["epoch"] == 2
    assert _same_state(net, syn_run["net"]) and _same_adam(opt, syn_run["out"]["optimizer"])
    assert opt.param_groups[0]["lr"] == syn_run["out"]["lr"][1]


def test_resume_is_bitwise(syn_run, tmp_path):
    """Two epochs straight == one epoch, checkpoint, resume, one epoch: bitwise in parameters and Adam state.

    This holds because the step itself repeats bit for bit: the one sum of the test network whose order was not fixed -- the bias gradient
    of the transposed convolution, four column partials per channel meeting through fp32 atomic adds -- is reduced in a fixed order
    (csrc/wgrad_f16.hip colpart_reduce_kernel)."""
    net = _net()
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()                                                              # (everything must come from the checkpoint)
    out = fit.fit_denoising(net, syn_run["pool"], CFG, resume=syn_run["out"]["checkpoints"][0], save_dir=tmp_path, log=lambda s: None)
    assert out["epoch_start"] == 1 and out["lr"] == syn_run["out"]["lr"][1:] and all(np.isnan(v) for v in out["psnr"])
    assert np.array_equal(out["rows"].view(np.uint32), syn_run["out"]["rows"][3:].view(np.uint32))
    assert out["train"] == syn_run["out"]["train"][1:]
    assert _same_state(net, syn_run["net"])
    final_a, final_b = torch.load(out["checkpoints"][0], map_location="cpu"), torch.load(syn_run["out"]["checkpoints"][1], map_location="cpu")
    assert final_a["epoch"] == final_b["epoch"] == 2
    assert all(torch.equal(final_a["model_state_dict"][k], v) for k, v in final_b["model_state_dict"].items())
    assert _same_adam(out["optimizer"], syn_run["out"]["optimizer"])


@pytest.mark.parametrize("c,cvalid,nblk", [(32, 32, 5), (64, 61, 700), (96, 96, 4161)])
def test_bias_sums_repeat_bit_for_bit(c, cvalid, nblk):
    """The column-partial reduction behind every bias gradient of the f16 pipe (what makes the step above repeat): the fp64 sum within
    fp32 summation error -- nblk terms of |x| < 1 in chains of nblk / 256 and a tree of 8 levels, so nblk * 2^-24 * (nblk / 256 + 9) is a
    bound -- and the same bits on every call, at one block per thread, a partly filled stride and several strides."""
    from virnet_amd import ops
    g = np.random.default_rng(c + nblk)
    col = torch.from_numpy(g.uniform(-1.0, 1.0, (c // 32, nblk, 32)).astype(np.float32)).cuda()
    want = col.double().sum(1).reshape(-1)[:cvalid]
    got = [ops.TImage(None, 1, 1, 1, c, False, col=col.reshape(-1), nblk=nblk, ncol=cvalid).bias_sums() for _ in range(3)]
    assert got[0].shape == (cvalid,) and torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    err = float((got[0].double() - want).abs().max())
    print("max |error|", err)
    assert err <= nblk * 2.0 ** -24 * (nblk / 256 + 9)


def test_transposed_conv_gradients_repeat_bit_for_bit():
    """The layer whose bias gradient used to differ from run to run: both column phases and two slices met in one channel."""
    from virnet_amd import ops
    g = np.random.default_rng(12)
    x = torch.from_numpy(g.standard_normal((4, 16, 16, 64)).astype(np.float32)).cuda()
    dy = torch.from_numpy(g.standard_normal((4, 32, 32, 32)).astype(np.float32)).cuda()
    runs = [ops.convt_wgrad(x, dy, (64, 32, 2, 2)) for _ in range(3)]
    assert all(torch.equal(runs[0][0], r[0]) and torch.equal(runs[0][1], r[1]) for r in runs[1:])
    want = dy.double().sum((0, 1, 2))
    assert float((runs[0][1].double() - want).abs().max()) <= 2e-5 * float(want.abs().max())          # (tests/test_backward_gpu.py's bar)


def test_no_host_synchronisation_between_two_log_reads(syn_run):
    pool, c = syn_run["pool"], fit.read_config(CFG)
    net = _net()
    p_r, p_s = fit.clip_sets(net)
    opt = ClipAdam(net.parameters(), lr=1e-4, clip=[(p_r, 1e3), (p_s, 1e2)])
    alpha0 = (0.5 * torch.tensor([49.0], dtype=torch.float32)).cuda()
    log = trainlog.StepLog(fit.LOG_NAMES, 8, 3)
    rng = random.Random(0)
    net.train()
    for ii in range(2):                                                            # the warm-up: plans, packed weights, cached tables
        fit.train_step(net, opt, pool, c, rng, 0, ii, alpha0, False, log)
    assert log.read()[0].shape == (2, 6)
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for ii in range(2, 5):
            fit.train_step(net, opt, pool, c, rng, 0, ii, alpha0, False, log)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    rows, _ = log.read()
    assert rows.shape == (3, 6) and np.isfinite(rows).all()


def test_validation_stage_equals_the_host_metrics(syn_run):
    """PSNR: the same double as eval.calculate_psnr on the same outputs; SSIM within the 1e-10 that virnet_amd/metrics.py promises for
    the device path against the host (eval.denoise_table's docstring: "SSIM within 1e-10")."""
    net, val, out = syn_run["net"], syn_run["val"], syn_run["out"]
    ims = _val_images()
    net.eval()
    psnrs, ssims = [], []
    with torch.no_grad():
        for i, gt in enumerate(ims):
            noisy, _ = val.batch([i])
            mu = net(noisy)[0]
            den = veval.img_as_ubyte(np.clip(mu[0].cpu().numpy().transpose(1, 2, 0), 0.0, 1.0))
            psnrs.append(veval.calculate_psnr(den, gt))
            ssims.append(veval.calculate_ssim(den, gt))
    got_psnr, got_ssim = out["val_images"][-1]
    print("psnr", got_psnr, psnrs, "ssim", got_ssim, ssims)
    assert got_psnr == psnrs
    assert max(abs(a - b) for a, b in zip(got_ssim, ssims)) <= 1e-10
    assert out["psnr"][-1] == float(np.mean(psnrs)) and abs(out["ssim"][-1] - float(np.mean(ssims))) <= 1e-10
    assert len(out["psnr"]) == 2 and any(line.startswith("test: PSNR=") for line in syn_run["lines"])
