"""CPU-side checks of the weight average (virnet_amd/ema.py, csrc/ema.hip, the ``ema_*`` keys of virnet_amd/fit.py): the bindings and the
argument errors (all raised before any device work), the numpy definition against fp64, the update's fixpoint, ``decay_at`` and the
weight's rounding, the state round trip on CPU parameters, the config readers, the checkpoint's key sets and ``model_state_of``.  No
kernel runs here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import ema_cases as ec
from conftest import REPO
from virnet_amd import _native, ema, fit, optim
from virnet_amd.ema import WeightEMA, decay_at, ema_np, weight_at

NEW_SYMBOLS = ("virnet_ema_update", "virnet_ema_swap")
DECAYS = (0.0, 0.5, 0.9, 0.999, 0.9999)


def test_symbols_are_bound_declared_and_the_abi_version_is_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    header = open(os.path.join(REPO, "include", "virnet_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
        assert f"int {name}(" in header
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5 and "#define VIRNET_ABI_VERSION 5\n" in header
    block = header[header.index("csrc/ema.hip"):header.index("int virnet_ema_update(")]
    assert "Additive under ABI version 5" in block
    assert optim.WeightEMA is WeightEMA


def test_bad_arguments_are_refused_before_any_launch():
    lib = _native.load()
    ptrs, one = (C.c_void_p * 2)(4096, 8192), (C.c_longlong * 2)(4, 4)
    calls = {"virnet_ema_update": lambda a, b, n, c: lib.virnet_ema_update(a, b, n, c, 0.25, None),
             "virnet_ema_swap": lambda a, b, n, c: lib.virnet_ema_swap(a, b, n, c, None)}
    for name, call in calls.items():
        assert call(None, None, None, 0) == 0 and call(ptrs, ptrs, one, 0) == 0          # count == 0: a no-op
        for args in ((None, ptrs, one, 2), (ptrs, None, one, 2), (ptrs, ptrs, None, 2)):
            assert call(*args) != 0 and b"NULL list" in lib.virnet_last_error() and name.encode() in lib.virnet_last_error()
        assert call(ptrs, ptrs, one, -1) != 0 and b"count -1" in lib.virnet_last_error()
        for bad in (0, -3, 1 << 31, 1 << 40):
            assert call(ptrs, (C.c_void_p * 2)(12288, 16384), (C.c_longlong * 2)(4, bad), 2) != 0
            assert b"tensor 1 has" in lib.virnet_last_error() and b"1 .. 2^31 - 1 expected" in lib.virnet_last_error()
        assert call((C.c_void_p * 1)(4098), (C.c_void_p * 1)(8192), one, 1) != 0 and b"misaligned" in lib.virnet_last_error()
        assert call((C.c_void_p * 1)(0), (C.c_void_p * 1)(8192), one, 1) != 0 and b"NULL" in lib.virnet_last_error()
        assert call((C.c_void_p * 1)(4096), (C.c_void_p * 1)(4096), one, 1) != 0 and b"the same" in lib.virnet_last_error()
    for w in (-0.5, 1.5, float("nan")):
        assert lib.virnet_ema_update(ptrs, (C.c_void_p * 2)(12288, 16384), one, 2, w, None) != 0 and b"weight" in lib.virnet_last_error()


def test_ema_np_is_within_three_roundings_of_fp64():
    """|ema_np - fp64| <= 2^-23 (|w (p - e)| + |e'|) elementwise: with u = 2^-24 the difference, the product and the sum are each off by at
    most u relatively, so the error is at most |t| ((1 + u)^2 - 1) (1 + u) + |e'| u + ... <= 2 u (|t| + |e'|) to first order."""
    g = np.random.default_rng(3)
    n = 1_000_000
    worst = 0.0
    for decay in DECAYS:
        w = weight_at(0, decay)
        e, p = ((10.0 ** g.uniform(-6, 2, n) * g.choice([-1.0, 1.0], n)).astype(np.float32) for _ in range(2))
        e[::7] = p[::7]
        p[3::11] = 0.0
        got = ema_np(e, p, w).astype(np.float64)
        t = float(w) * (p.astype(np.float64) - e.astype(np.float64))
        want = e.astype(np.float64) + t
        bound = 2.0 ** -23 * (np.abs(t) + np.abs(want))
        err = np.abs(got - want)
        assert (err <= bound).all(), (decay, float((err - bound).max()))
        ratio = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))
        worst = max(worst, ratio)
    print(f"ema_np against fp64: worst error / bound {worst:.3f}")


def test_the_fixpoint_is_exact_and_ema_np_takes_float32_only():
    ps, es = ec.values(0)
    for decay in DECAYS:
        w = weight_at(0, decay)
        for i, (p, e) in enumerate(zip(ps, es)):
            with np.errstate(invalid="ignore"):
                out = ema_np(p.numpy(), p.numpy(), w)                      # p == e everywhere (the NaN and Inf - Inf aside)
            keep = np.isfinite(p.numpy())
            assert np.array_equal(out.view(np.uint32)[keep], p.numpy().view(np.uint32)[keep])
            mask = ec.fixpoints(i).numpy()
            with np.errstate(invalid="ignore", over="ignore"):
                out = ema_np(e.numpy(), p.numpy(), w)
            assert mask.sum() == len(range(ec.ALL_SIZES[i])[(3 - i) % 7::7])
            assert np.array_equal(out.view(np.uint32)[mask], e.numpy().view(np.uint32)[mask])
    assert ema_np(np.float32([1.0]), np.float32([3.0]), 0.25).dtype == np.float32 and ema_np(np.float32([1.0]), np.float32([3.0]), 0.25)[0] == 1.5
    with pytest.raises(TypeError, match="float32"):
        ema_np(np.zeros(3), np.zeros(3, dtype=np.float32), 0.5)


def test_decay_at_and_the_weight_is_rounded_once():
    assert decay_at(0, 0.999) == decay_at(10 ** 6, 0.999) == 0.999
    assert [decay_at(t, 0.999, True) for t in (0, 1, 2, 90)] == [1.0 / 10.0, 2.0 / 11.0, 3.0 / 12.0, 91.0 / 100.0]
    assert decay_at(8989, 0.999, True) == 8990.0 / 8999.0 < 0.999 and decay_at(8991, 0.999, True) == 0.999 == decay_at(10 ** 7, 0.999, True)
    assert decay_at(5, 0.05, True) == 0.05
    for t, decay, warm in ((0, 0.999, False), (0, 0.999, True), (1, 0.9999, True), (7, 0.9, False)):
        w = weight_at(t, decay, warm)
        assert w == float(np.float32(1.0 - decay_at(t, decay, warm))) and np.float32(w) == w
    assert weight_at(0, 0.999) != float(np.float32(1.0) - np.float32(0.999))          # (the difference is formed in doubles, then rounded)
    assert weight_at(0, 0.0) == 1.0 and weight_at(0, 0.5) == 0.5
    e = WeightEMA([("a", torch.nn.Parameter(torch.zeros(3)))], decay=0.99, warmup=True)
    assert e.decay_at() == 0.1 and e.decay_at(1000) == 0.99 and e.num_updates == 0 and e.swapped is False
    for bad in (1.0, -0.1, 1.5, float("nan"), True, "0.9", torch.tensor(0.9)):
        with pytest.raises(ValueError, match="decay"):
            WeightEMA([("a", torch.nn.Parameter(torch.zeros(3)))], decay=bad)


def _module():
    torch.manual_seed(5)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.PReLU(), torch.nn.Conv2d(4, 2, 1, bias=False))


def test_state_round_trip_on_cpu_and_no_cpu_fallback():
    net = _module()
    avg = WeightEMA(net, decay=0.9, warmup=True)
    assert avg.names == list(net.state_dict()) and all(torch.equal(s, p) and s.data_ptr() != p.data_ptr() for s, p in zip(avg.shadows, avg.params))
    assert all(not s.requires_grad for s in avg.shadows)
    before = [p.detach().clone() for p in net.parameters()]
    for call in (avg.update, avg.swap):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with avg.averaged():
            pass
    assert avg.num_updates == 0 and avg.swapped is False and all(torch.equal(p, q) for p, q in zip(net.parameters(), before))
    sd = avg.state_dict()
    assert set(sd) == {"decay", "warmup", "num_updates", "shadow"} and (sd["decay"], sd["warmup"], sd["num_updates"]) == (0.9, True, 0)
    assert list(sd["shadow"]) == list(net.state_dict()) == list(avg.model_state_dict())
    fresh = _module()
    fresh.load_state_dict(avg.model_state_dict(), strict=True)                 # model format
    sd["shadow"] = {k: v + 1.0 for k, v in sd["shadow"].items()}
    sd["num_updates"], sd["decay"], sd["warmup"] = 17, 0.75, False
    other = WeightEMA(_module())
    other.load_state_dict(sd)
    assert (other.decay, other.warmup, other.num_updates) == (0.75, False, 17)
    assert all(torch.equal(s, v) and s.data_ptr() != v.data_ptr() for s, v in zip(other.shadows, sd["shadow"].values()))
    back = other.state_dict()
    assert {k: back[k] for k in ("decay", "warmup", "num_updates")} == {k: sd[k] for k in ("decay", "warmup", "num_updates")}
    assert all(torch.equal(back["shadow"][k], v) for k, v in sd["shadow"].items())
    other.load_state_dict(dict(sd, shadow={"module." + k: v for k, v in sd["shadow"].items()}))          # a DistributedDataParallel prefix
    with pytest.raises(KeyError, match="missing"):
        other.load_state_dict(dict(sd, shadow={k: v for k, v in list(sd["shadow"].items())[1:]}))
    with pytest.raises(KeyError, match="num_updates"):
        other.load_state_dict({k: v for k, v in sd.items() if k != "num_updates"})
    with pytest.raises(ValueError, match="float32 expected"):
        other.load_state_dict(dict(sd, shadow={k: v.double() for k, v in sd["shadow"].items()}))
    with pytest.raises(TypeError, match="float32"):
        WeightEMA(_module().half())
    with pytest.raises(TypeError, match="name, parameter"):
        WeightEMA(list(net.parameters()))
    with pytest.raises(ValueError, match="contiguous"):
        WeightEMA([("w", torch.nn.Parameter(torch.zeros(4, 6).t()))])


DENOISE_CFG = dict(batch_size=16, patch_size=128, epochs=120, warmup_epochs=5, lr=1e-4, clip_grad_R=1e3, clip_grad_S=1e2, var_window=7, eps2=1e-6)


@pytest.mark.parametrize("reader", ["read_config", "read_sisr_config"])
def test_config_readers_take_the_new_keys(reader):
    cfg = DENOISE_CFG if reader == "read_config" else fit.load_config(os.path.join(REPO, "tests", "golden", "configs", "sisr_x4.json"))
    read = getattr(fit, reader)
    off = read(cfg)
    assert off["ema_decay"] is None and off["ema_warmup"] is False
    for none in (None, 0, 0.0):
        assert read(dict(cfg, ema_decay=none))["ema_decay"] is None
    c = read(dict(cfg, ema_decay=0.999))
    assert c["ema_decay"] == 0.999 and c["ema_warmup"] is False
    for spelled, want in ((True, True), (False, False), ("True", True), ("False", False), ("true", True)):
        assert read(dict(cfg, ema_decay=0.5, ema_warmup=spelled))["ema_warmup"] is want
    for bad in (1.0, -0.5, 2, "0.999", True, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            read(dict(cfg, ema_decay=bad))
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="ema_warmup"):
            read(dict(cfg, ema_decay=0.9, ema_warmup=bad))
    assert {k: v for k, v in off.items() if not k.startswith("ema_")} == {k: v for k, v in c.items() if not k.startswith("ema_")}


def test_checkpoint_keys_without_the_average_are_todays_and_model_state_of():
    net = _module()
    opt = torch.optim.Adam(net.parameters())
    plain = fit.checkpoint_dict(net, opt, 1, 5, {"train": 1, "test": 2})
    assert set(plain) == {"epoch", "step", "step_img", "model_state_dict", "optimizer_state_dict"}
    assert set(fit.checkpoint_dict(net, None, 1, 5, {"train": 1, "test": 2})) == {"epoch", "step", "step_img", "model_state_dict"}
    avg = WeightEMA(net, decay=0.9)
    with torch.no_grad():
        for s in avg.shadows:
            s.add_(1.0)
    avg.num_updates = 4
    ckpt = fit.checkpoint_dict(net, opt, 1, 5, {"train": 1, "test": 2}, ema=avg)
    assert set(ckpt) == set(plain) | {"ema_state_dict", "ema"} and ckpt["ema"] == {"decay": 0.9, "warmup": False, "num_updates": 4}
    assert fit.model_state_of(ckpt) is ckpt["model_state_dict"] and fit.model_state_of(ckpt, ema=True) is ckpt["ema_state_dict"]
    assert fit.model_state_of(plain) is plain["model_state_dict"]
    with pytest.raises(KeyError, match="ema_state_dict"):
        fit.model_state_of(plain, ema=True)
    with pytest.raises(KeyError, match="model_state_dict"):
        fit.model_state_of({"epoch": 1})
    assert list(ckpt["ema_state_dict"]) == list(ckpt["model_state_dict"])
    assert all(torch.equal(ckpt["ema_state_dict"][k], v + 1.0) for k, v in ckpt["model_state_dict"].items())
    # today's callers ignore the two keys; a loader that knows them restores both, one without them starts at the loaded parameters
    a, b = _module(), _module()
    with torch.no_grad():
        for p in list(a.parameters()) + list(b.parameters()):
            p.zero_()
    assert fit.load_checkpoint(ckpt, a)["epoch"] == 1 and all(torch.equal(p, q) for p, q in zip(a.parameters(), net.parameters()))
    avg_b = WeightEMA(b, decay=0.5, warmup=True)
    fit.load_checkpoint(ckpt, b, ema=avg_b)
    assert (avg_b.decay, avg_b.warmup, avg_b.num_updates) == (0.5, True, 4)                  # (decay and warm-up are the run's configuration)
    assert all(torch.equal(s, v) for s, v in zip(avg_b.shadows, ckpt["ema_state_dict"].values()))
    avg_b.num_updates = 9
    fit.load_checkpoint(plain, b, ema=avg_b)
    assert avg_b.num_updates == 0 and all(torch.equal(s, p) for s, p in zip(avg_b.shadows, net.parameters()))


# ---- the drivers' flags ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tc():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import train_common
        yield train_common
    finally:
        sys.path.remove(os.path.join(REPO, "tools"))


def test_the_drivers_flags_override_the_config(tc):
    parse = lambda argv: tc.parse_flags(argv, "d.json", "./rec", "help")
    assert (parse([]).ema_decay, parse([]).ema_warmup) == (None, None)
    opts = parse(["--ema-decay", "0.999", "--ema-warmup", "--gpus", "2"])
    assert (opts.ema_decay, opts.ema_warmup, opts.gpus) == (0.999, True, 2)
    for bad in ("1", "-0.1", "x"):
        with pytest.raises(SystemExit):
            parse(["--ema-decay", bad])
    cfg = dict(DENOISE_CFG, ema_decay=0.5, ema_warmup="False")
    assert tc.apply_ema_flags(dict(cfg), parse([])) == cfg                                   # no flag: the config stands
    got = fit.read_config(tc.apply_ema_flags(dict(cfg), opts))
    assert (got["ema_decay"], got["ema_warmup"]) == (0.999, True)
    assert fit.read_config(tc.apply_ema_flags(dict(cfg), parse(["--ema-decay", "0"])))["ema_decay"] is None      # 0 switches it off
    # the ranks of --gpus N are started with the flags still in place
    cmds = tc.rank_commands(2, "/x/train.py", ["--ema-decay", "0.999", "--gpus", "2", "--ema-warmup"], 2345, environ={})
    assert all(cmd[2:] == ["--ema-decay", "0.999", "--ema-warmup"] for cmd, _ in cmds)
