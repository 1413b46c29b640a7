"""The host side of the multi-rank fit loops (virnet_amd/fit.py, tools/train_common.py), no GPU: which rows a rank synthesises, the
real-noise partner selection against the numpy definition of the batch, rank 0 alone logging, and the drivers' ``--gpus`` flag."""
import glob
import os
import random
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from virnet_amd import datagen, fit
from virnet_amd import eval as veval


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [4, 6, 8])
@pytest.mark.parametrize("world", [1, 2, 4])
def test_ranks_rows_are_disjoint_and_cover_the_batch_in_order(batch, world):
    if batch % world:
        with pytest.raises(ValueError, match=f"{batch}.*world size {world}"):
            fit.shard_rows(batch, world, 0)
        return
    rows = []
    for rank in range(world):
        a, b = fit.shard_rows(batch, world, rank)
        assert b - a == batch // world
        rows += list(range(a, b))
    assert rows == list(range(batch))


def test_batch_six_world_four_raises():
    with pytest.raises(ValueError, match="6.*world size 4"):
        fit.shard_rows(6, 4, 1)


# ---- the real-noise partner selection ----------------------------------------------------------------------------------------------------------
def _pairs():
    files = sorted(glob.glob(os.path.join(GOLDEN, "cbsd68", "*.png")))
    assert len(files) >= 8
    noisy = [veval.imread_rgb_uint8(f) for f in files[:4]]
    return noisy, [np.ascontiguousarray(a[::-1, ::-1]) for a in noisy]          # (any second image of the same size serves as ground truth)


@pytest.mark.parametrize("world", [2, 4])
def test_partner_selection_gives_the_rows_of_the_whole_batch(world):
    noisy, gt = _pairs()
    batch, p = 8, 24
    params = datagen.draw_pair_params(random.Random(3), noisy, batch, p)
    perm = np.array([5, 0, 7, 1, 2, 6, 3, 4])                  # a permutation whose pairs cross the shard boundaries of both world sizes
    lam = np.linspace(0.1, 0.9, batch).astype(np.float32)
    mix = datagen.MixParams(perm, lam)
    full = datagen.real_batch_np(noisy, gt, params, mix)
    for rank in range(world):
        a, b = fit.shard_rows(batch, world, rank)
        n = b - a
        assert any(not a <= perm[i] < b for i in range(a, b))  # a partner lives on another rank
        sel_params, sel_mix = fit.shard_real_params(params, mix, a, b)
        assert sel_params.n == sel_mix.n == 2 * n
        assert list(sel_mix.perm[:n]) == list(range(n, 2 * n)) and list(sel_mix.perm[n:]) == list(range(n, 2 * n))      # partners pair with themselves
        part = datagen.real_batch_np(noisy, gt, sel_params, sel_mix)
        for whole, mine in zip(full, part):
            assert mine.dtype == np.float32 and mine[:n].tobytes() == whole[a:b].tobytes()


# ---- logging -----------------------------------------------------------------------------------------------------------------------------------
def test_only_rank_zero_logs(monkeypatch):
    """``_fit`` up to its first device work, with the world faked: rank 1's ``log`` never fires, rank 0's does (the resume line is the
    first thing the loop says)."""
    import torch.distributed as tdist
    seen = {}

    class Stop(Exception):
        pass

    def fake_load(path, net, opt, map_location=None):
        return {"epoch": 0, "step": 0}

    def stop(*a, **k):
        raise Stop

    monkeypatch.setattr(fit, "load_checkpoint", fake_load)
    monkeypatch.setattr(fit, "_optimizer", lambda net, c, keys: None)
    monkeypatch.setattr(datagen, "_require_device", lambda device, who: torch.device("cpu"))
    net = torch.nn.Linear(2, 2)
    pool = datagen.ImagePool.__new__(datagen.ImagePool)
    pool.device, pool.data_b = torch.device("cpu"), None
    cfg = dict(batch_size=4, patch_size=8, epochs=1, warmup_epochs=0, lr=1e-4, clip_grad_R=1.0, clip_grad_S=1.0, var_window=7, eps2=1e-6)
    for rank in (0, 1):
        monkeypatch.setattr(fit, "_world", lambda group, rank=rank: (2, rank))
        monkeypatch.setattr(fit, "Shard", stop)                # (the last host-only thing before the loop touches the device)
        import virnet_amd.dist as vdist
        monkeypatch.setattr(vdist, "broadcast_parameters", lambda *a, **k: 0)
        monkeypatch.setattr(vdist, "GradientReducer", lambda *a, **k: object())
        lines = []
        with pytest.raises(Stop):
            fit.fit_denoising(net, pool, cfg, resume={"epoch": 0}, log=lines.append)
        seen[rank] = lines
        if hasattr(net, "_grad_reducer"):
            del net._grad_reducer
    assert seen[0] == ["=> Loaded checkpoint <dict> (epoch 0)"] and seen[1] == []
    assert not tdist.is_initialized()


# ---- the drivers' flag -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tc():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import train_common
        yield train_common
    finally:
        sys.path.remove(os.path.join(REPO, "tools"))


def test_gpus_flag_is_parsed(tc):
    opts = tc.parse_flags(["--config", "c.json", "--gpus", "8"], "d.json", "./rec", "help")
    assert (opts.gpus, opts.config, opts.save_dir, opts.resume) == (8, "c.json", "./rec", None)
    assert tc.parse_flags([], "d.json", "./rec", "help").gpus is None
    for bad in ("0", "17", "two"):
        with pytest.raises(SystemExit):
            tc.parse_flags(["--gpus", bad], "d.json", "./rec", "help")


def test_rank_commands_are_fresh_processes_under_the_torchrun_variables(tc):
    cmds = tc.rank_commands(3, "/x/train.py", ["--config", "c.json", "--gpus", "3", "--resume", "m.pth", "--gpus=3"], 2345, environ={"A": "b", "RANK": "9"})
    assert len(cmds) == 3
    for r, (cmd, env) in enumerate(cmds):
        assert cmd == [sys.executable, "/x/train.py", "--config", "c.json", "--resume", "m.pth"]      # the flag is gone: a child never spawns again
        assert (env["RANK"], env["LOCAL_RANK"], env["WORLD_SIZE"], env["MASTER_ADDR"], env["MASTER_PORT"], env["A"]) == (str(r), str(r), "3", "127.0.0.1", "2345", "b")
    with pytest.raises(ValueError):
        tc.rank_commands(17, "/x/train.py", [], 1)


def test_init_passes_a_timeout_through(monkeypatch):
    import datetime
    import virnet_amd.dist as vdist
    seen = {}
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")
    monkeypatch.setattr(vdist.dist, "init_process_group", lambda **kw: seen.update(kw))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert vdist.init(backend="gloo", timeout=120) == (1, 1, 2)
    assert seen["timeout"] == datetime.timedelta(seconds=120) and seen["backend"] == "gloo" and seen["world_size"] == 2
    seen.clear()
    vdist.init(backend="gloo")
    assert "timeout" not in seen
