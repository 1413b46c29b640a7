"""Host-side checks of the device training loop's pieces (virnet_amd/schedule.py, datagen.SimulateTestSet, trainlog.StepLog, fit.py): the
learning rates are the reference's own doubles (tests/golden/lr_schedule.json, made by tests/golden/make_lr_schedule_golden.py), the numpy
definition of the validation set is the reference's ``SimulateTest`` bit for bit (tests/golden/simulate_test.npz, made by
tests/golden/make_simulate_test_golden.py), the nearest-exact index tables are ``eval.resize_nearest_exact``'s and the written rule's, the
config reader strips ``#`` comments outside strings only, the C entries are bound at ABI version 5, and argument errors are raised before
any device work."""
import ctypes as C
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import datagen_cases as dc
from conftest import GOLDEN, REPO, load_golden
from test_kernel_resources import _remarks, _table
from virnet_amd import _native, datagen, fit, schedule, trainlog
from virnet_amd import eval as veval
from virnet_amd.optim import ClipAdam

NEW_SYMBOLS = ("virnet_datagen_simulate_test", "virnet_trainlog_bytes", "virnet_trainlog_push", "virnet_trainlog_reset")


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------------
def _lr_cases():
    with open(os.path.join(GOLDEN, "lr_schedule.json")) as f:
        return json.load(f)["cases"]


def test_the_schedule_is_the_reference_double_for_double():
    """The recursion is at most ~150 steps of a few Python double operations written in the reference's order: it is bit-identical, so
    equality of the doubles is asserted (no tolerance)."""
    cases = _lr_cases()
    assert {(8, 2), (120, 5), (6, 0)} <= {(c["epochs"], c["warmup_epochs"]) for c in cases}
    for c in cases:
        got = schedule.warmup_cosine(c["lr"], c["lr_min"], c["epochs"], c["warmup_epochs"])
        assert len(got) == c["epochs"] and got == c["lrs"], (c["epochs"], c["warmup_epochs"])
        for epoch, lr in c["replayed"].items():          # resuming = indexing: the reference replays scheduler.step() `epoch` times
            assert got[int(epoch)] == lr


def test_the_schedule_overshoots_after_the_warm_up_and_is_not_the_textbook_curve():
    got = schedule.warmup_cosine(1e-4, 1e-6, 8, 2)
    assert got[0] == 5e-05 and got[1] == 1e-4 and got[2] > 1e-4 and got[3] == pytest.approx(1e-4, rel=1e-12)
    assert got[2] == pytest.approx(1.0710788e-04, rel=1e-7)
    assert all(a > b for a, b in zip(got[2:], got[3:]))
    for bad in ((8, 8), (8, 9), (0, 0), (8, -1), (8.5, 2)):
        with pytest.raises(ValueError):
            schedule.warmup_cosine(1e-4, 1e-6, *bad)


# ---- the validation set ------------------------------------------------------------------------------------------------------------------------
def test_simulate_test_np_is_the_reference_bit_for_bit():
    G = load_golden("simulate_test")
    ims = [G["u8_0"], G["u8_1"]]
    assert [i.shape for i in ims] == [(40, 56, 3), (56, 40, 3)] and G["noise"].shape == (56, 56, 3)
    assert dc.same_bits(datagen.simulate_noise([i.shape[:2] for i in ims], int(G["seed"])), G["noise"])
    assert dc.same_bits(datagen.simulate_sigma_map(), G["sigma_map"])
    for i in range(2):
        noisy, gt = datagen.simulate_test_np(ims, [i], G["noise"], G["sigma_map"])
        assert dc.same_bits(noisy[0], G[f"noisy_{i}"]) and dc.same_bits(gt[0], G[f"gt_{i}"])
    # the bar discriminates: the training set's u8 * fp32(1/255) is another float for 126 byte values, a fused multiply-add another sum
    assert not dc.same_bits(np.ascontiguousarray(datagen.u8_to_float_np(ims[0]).transpose(2, 0, 1)), G["gt_0"])
    sigma = veval.resize_nearest_exact(G["sigma_map"], 40, 56)[:, :, None].astype(np.float64)
    fused = (G["gt_0"].transpose(1, 2, 0).astype(np.float64) + G["noise"][:40, :56].astype(np.float64) * sigma).astype(np.float32)
    assert not dc.same_bits(np.ascontiguousarray(fused.transpose(2, 0, 1)), G["noisy_0"])
    with pytest.raises(ValueError):
        datagen.simulate_test_np(ims, [0, 1], G["noise"], G["sigma_map"])


@pytest.mark.parametrize("size", [1, 7, 255, 256, 257, 300])
def test_index_tables_are_resize_nearest_exact(size):
    idx = datagen.nearest_exact_indices(size)
    assert idx.dtype == np.int32 and idx.shape == (size,) and idx.min() >= 0 and idx.max() <= 255
    a = np.arange(256 * 256, dtype=np.int64).reshape(256, 256)
    assert np.array_equal(veval.resize_nearest_exact(a, size, 3)[:, 0] // 256, idx)
    assert np.array_equal(veval.resize_nearest_exact(a, 3, size)[0] % 256, idx)
    # the written rule, in exact arithmetic: floor((dst + 0.5) * 256 / size)
    assert idx.tolist() == [min((Fraction(2 * d + 1, 2) * 256 / size).__floor__(), 255) for d in range(size)]


def test_simulate_test_set_refusals_come_before_any_device_work():
    ims = [np.zeros((12, 16, 3), np.uint8), np.zeros((16, 12, 3), np.uint8), np.zeros((12, 16, 3), np.uint8)]
    with pytest.raises(TypeError, match="ImagePool"):
        datagen.SimulateTestSet(ims)
    pool = datagen.ImagePool(ims, "cpu")
    with pytest.raises(TypeError, match="seed"):
        datagen.SimulateTestSet(pool, seed=1.5)
    vs = datagen.SimulateTestSet(pool)
    assert vs.noise_np.shape == (16, 16, 3) and vs.groups() == [[0, 2], [1]] and len(vs) == 3
    with pytest.raises(ValueError, match="one shape"):
        vs.batch([0, 1])
    with pytest.raises(ValueError, match=r"indices\[1\] = 3 outside"):
        vs.batch([0, 3])
    with pytest.raises(ValueError, match="indices"):
        vs.batch([])
    with pytest.raises(TypeError, match="indices"):
        vs.batch(torch.tensor([0]))
    with pytest.raises(TypeError, match=r"indices\[0\]"):
        vs.batch([0.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vs.batch([0, 2, 0])


# ---- the config reader -----------------------------------------------------------------------------------------------------------------------
def test_comment_stripper_respects_strings():
    text = '{\n  # a comment line with "quotes" and a brace }\n  "lr": 1e-4,   # after a value\n  "path": "/data/#1/set # not a comment",\n' \
           '  "esc": "a \\" # still inside \\\\",  # outside\n  "n_feat": [96, 192] # end\n}\n'
    got = json.loads(fit.strip_json_comments(text))
    assert got == {"lr": 1e-4, "path": "/data/#1/set # not a comment", "esc": 'a " # still inside \\', "n_feat": [96, 192]}
    assert fit.strip_json_comments('{"a": 1}') == '{"a": 1}'


def test_read_config_checks_the_reference_keys():
    cfg = dict(batch_size=16, patch_size=128, epochs=120, warmup_epochs=5, lr=1e-4, lr_min=1e-6, print_freq=100, clip_grad_R=1e3, clip_grad_S=1e2,
               var_window=7, eps2=1e-6, im_chn=3, n_feat=[96, 192, 288])
    c = fit.read_config(cfg)
    assert c["steps_per_epoch"] == 10000 and c["batch_size"] == 16 and c["lr_min"] == 1e-6 and "n_feat" not in c
    del cfg["lr_min"]
    assert fit.read_config(cfg)["lr_min"] == 1e-6          # (train_denoising_real.py hard-codes it)
    with pytest.raises(KeyError, match="eps2"):
        fit.read_config({k: v for k, v in cfg.items() if k != "eps2"})
    with pytest.raises(ValueError, match="batch_size"):
        fit.read_config(dict(cfg, batch_size=0))
    with pytest.raises(ValueError, match="warmup_epochs"):
        fit.read_config(dict(cfg, warmup_epochs=120))


@pytest.mark.parametrize("reader", ["read_config", "read_sisr_config"])
def test_both_readers_refuse_the_same_things_the_same_way(reader):
    """What the two readers share by construction (one typed loop, ``fit._read``): a string for an integer key and a bool for a float key
    are ValueErrors that name the key and the type, a missing key is a KeyError that names it, and a non-dict a TypeError."""
    if reader == "read_config":
        cfg = dict(batch_size=16, patch_size=128, epochs=120, warmup_epochs=5, lr=1e-4, clip_grad_R=1e3, clip_grad_S=1e2, var_window=7, eps2=1e-6)
    else:
        cfg = fit.load_config(os.path.join(GOLDEN, "configs", "sisr_x4.json"))
    read = getattr(fit, reader)
    assert read(cfg)["batch_size"] == 16 and read(dict(cfg, batch_size=16.0, print_freq=7.0))["print_freq"] == 7
    for key in ("batch_size", "epochs", "var_window", "print_freq", "steps_per_epoch"):
        for bad in ("16", "", "sixteen"):
            with pytest.raises(ValueError, match=rf"cfg\['{key}'\] = '{bad}': a positive integer is expected"):
                read(dict(cfg, **{key: bad}))
        for bad in (True, 2.5, 0, -1):
            with pytest.raises(ValueError, match=rf"cfg\['{key}'\] = .*: a positive integer is expected"):
                read(dict(cfg, **{key: bad}))
    for key in ("lr", "lr_min", "clip_grad_R", "clip_grad_S", "eps2"):
        for bad in (True, False, "1e-4", -1e-4, float("nan")):
            with pytest.raises(ValueError, match=rf"cfg\['{key}'\] = .*: a non-negative float is expected"):
                read(dict(cfg, **{key: bad}))
    for key in ("eps2", "batch_size", "lr"):
        with pytest.raises(KeyError, match=key):
            read({k: v for k, v in cfg.items() if k != key})
    with pytest.raises(TypeError, match="must be a dict"):
        read(list(cfg.items()))
    if reader == "read_config":          # the one count that may be zero
        assert read(dict(cfg, warmup_epochs=0))["warmup_epochs"] == 0
        for bad in ("5", True, -1):
            with pytest.raises(ValueError, match=r"cfg\['warmup_epochs'\] = .*: a non-negative integer is expected"):
                read(dict(cfg, warmup_epochs=bad))


def test_log_lines_are_the_reference_format():
    line = fit.train_line(0, 120, 99, 10000, [1.5, -2.25, 3.125, 0.5, 1234.5, 0.02], 1e3, 1e2, 2e-5)
    assert line == "[Epoch: 1/120] train:00100/10000, lh=-2.25, KLG=+++3.12, KLIG=++0.50, GNorm_D:1.0e+03/1.2e+03, GNorm_S:1.0e+02/2.0e-02, lr=2.00e-05"
    assert fit.epoch_line([1.5, -2.25, 3.125, 0.5]) == "train: Loss=+1.50e+00, lh=-2.25e+00, KL_Guass=+3.12e+00, KLIG=+5.00e-01"


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_bound_and_abi_version_unchanged():
    lib = _native.load()
    bound = {name for name, _, _ in _native.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(lib, name) is not None
    assert _native.ABI_VERSION == 5 and lib.virnet_abi_version() == 5
    with open(os.path.join(REPO, "include", "virnet_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+VIRNET_ABI_VERSION\s+5\b", header)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, header)
    assert f"#define VIRNET_TRAINLOG_MAX {trainlog.MAX_VALUES}\n" in header and f"#define VIRNET_SIMTEST_MAP {datagen.SIMTEST_MAP}\n" in header
    assert f"#define VIRNET_TRAINLOG_MAX_CAPACITY {trainlog.MAX_CAPACITY}\n" in header


def test_the_c_entries_refuse_bad_arguments_before_any_launch():
    lib = _native.load()
    err = lambda: lib.virnet_last_error().decode()          # noqa: E731
    assert lib.virnet_trainlog_bytes(6, 8) == 6 * 8 + 8 * 6 * 4
    assert lib.virnet_trainlog_bytes(17, 8) == 0 and "k 17" in err()
    assert lib.virnet_trainlog_bytes(6, 0) == 0 and "capacity 0" in err()
    host = np.zeros(256, dtype=np.float64)          # (host memory: every call below is refused before it would launch)
    base = host.ctypes.data
    src, cnt = (C.c_void_p * 2)(base + 1024, base + 1028), (C.c_int * 2)(1, 2)
    assert lib.virnet_trainlog_push(src, cnt, 2, base, 17, 8, 0, 10, None) != 0 and "17 values" in err()
    assert lib.virnet_trainlog_push(src, cnt, 2, base, 3, 8, 8, 10, None) != 0 and "slot 8" in err()
    assert lib.virnet_trainlog_push(src, cnt, 2, base, 3, 8, 0, 0, None) != 0 and "num_iter" in err()
    assert lib.virnet_trainlog_push(src, cnt, 2, None, 3, 8, 0, 10, None) != 0 and "NULL" in err()
    assert lib.virnet_trainlog_push(src, cnt, 2, base + 4, 3, 8, 0, 10, None) != 0 and "aligned" in err()
    assert lib.virnet_trainlog_push(src, cnt, 2, base, 4, 8, 0, 10, None) != 0 and "hold 3 values" in err()
    assert lib.virnet_trainlog_push((C.c_void_p * 2)(base + 1024, base + 1030), cnt, 2, base, 3, 8, 0, 10, None) != 0 and "misaligned" in err()
    assert lib.virnet_trainlog_push((C.c_void_p * 2)(base + 1024, base + 16), cnt, 2, base, 3, 8, 0, 10, None) != 0 and "inside the log" in err()
    assert lib.virnet_trainlog_reset(None, 3, None) != 0 and "NULL" in err()
    p = [base + 256 * k for k in range(7)]
    out0, out1 = base + 256 * 7, base + 256 * 7 + 4 * 3 * 4 * 4
    args = lambda n=1, h=4, w=4, hm=8, wm=8, o0=out0, o1=out1: p + [n, h, w, hm, wm, o0, o1, None]          # noqa: E731
    sim = lib.virnet_datagen_simulate_test
    assert sim(*args(n=0)) != 0 and "images" in err()
    assert sim(*args(h=9)) != 0 and "outside the noise array" in err()
    assert sim(*args(w=9)) != 0 and "outside the noise array" in err()
    assert sim(*args(o1=None)) != 0 and "NULL" in err()
    assert sim(*args(o0=out0 + 2)) != 0 and "misaligned" in err()
    assert sim(*args(o1=out0 + 16)) != 0 and "overlap" in err()
    assert sim(*args(o0=p[3])) != 0 and "overlaps an input" in err()


def test_new_kernels_do_not_use_scratch():
    for unit, kernels in (("datagen", {"simulate_test_kernel"}), ("trainlog", {"trainlog_push_kernel", "trainlog_reset_kernel"})):
        rows = [r for r in _table(_remarks(unit)) if r["pretty"].replace("void ", "") in kernels]
        assert {r["pretty"].replace("void ", "") for r in rows} == kernels, [r["pretty"] for r in rows]
        for r in rows:
            assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r


# ---- the step log ----------------------------------------------------------------------------------------------------------------------------
def test_step_log_refusals_come_before_any_device_work():
    names = ["Loss", "lh", "KLG", "KLIG", "GNorm_R", "GNorm_S"]
    with pytest.raises(ValueError, match="17 values"):
        trainlog.StepLog([f"v{i}" for i in range(17)], 8, 10)
    with pytest.raises(ValueError, match="capacity"):
        trainlog.StepLog(names, 0, 10)
    with pytest.raises(ValueError, match="num_iter"):
        trainlog.StepLog(names, 8, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trainlog.StepLog(names, 8, 10, device="cpu")
    with pytest.raises(TypeError, match="names"):
        trainlog.StepLog([], 8, 10)
    log = trainlog.StepLog(names, 8, 10)
    s = torch.zeros(())
    with pytest.raises(RuntimeError, match=r"argument 0 \('Loss'\) is on cpu"):
        log.push(s, s, s, s, torch.zeros(2))
    with pytest.raises(TypeError, match=r"argument 1 \('lh'\) is torch.float64"):
        log.push(s, s.double(), s, s, torch.zeros(2))
    with pytest.raises(TypeError, match=r"argument 4 \('GNorm_R', 'GNorm_S'\) is torch.float16"):
        log.push(s, s, s, s, torch.zeros(2).half())
    with pytest.raises(ValueError, match=r"argument 4 brings the step to 7 values, the log holds k = 6"):
        log.push(s, s, s, s, torch.zeros(3))
    with pytest.raises(ValueError, match="hold 5 values"):
        log.push(s, s, s, s, s)
    with pytest.raises(ValueError, match=r"argument 2 has shape \(1, 1\)"):
        log.push(s, s, torch.zeros(1, 1), s, torch.zeros(2))
    with pytest.raises(TypeError, match="argument 3 must be a tensor"):
        log.push(s, s, s, 0.5, torch.zeros(2))
    many = trainlog.StepLog([f"v{i}" for i in range(16)], 8, 10)
    with pytest.raises(ValueError, match=r"argument 1 brings the step to 17 values, the log holds k = 16 \(.*at most 16\)"):
        many.push(torch.zeros(16), s)
    assert log.pushed == 0 and log._buf is None
    rows, sums = log.read()
    assert rows.shape == (0, 6) and sums.tolist() == [0.0] * 6


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------------------
def _tiny():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))


def test_checkpoint_keys_and_module_prefix_loading():
    net = _tiny()
    opt = ClipAdam(net.parameters(), lr=1e-4)
    ck = fit.checkpoint_dict(net, opt, 3, 41, {"train": 2, "test": 5, "other": 9})
    assert set(ck) == {"epoch", "step", "step_img", "model_state_dict", "optimizer_state_dict"}
    assert ck["epoch"] == 3 and ck["step"] == 41 and ck["step_img"] == {"train": 2, "test": 5}
    assert set(ck["model_state_dict"]) == set(net.state_dict()) and set(ck["optimizer_state_dict"]) == {"state", "param_groups"}
    assert set(fit.checkpoint_dict(net, None, 1, 1, {"train": 0, "test": 0})) == {"epoch", "step", "step_img", "model_state_dict"}
    # a DistributedDataParallel checkpoint: every key carries "module."
    other = _tiny()
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    prefixed = {"epoch": 3, "step": 41, "step_img": {"train": 0, "test": 0}, "model_state_dict": {"module." + k: v for k, v in ck["model_state_dict"].items()}}
    got = fit.load_checkpoint(prefixed, other, ClipAdam(other.parameters(), lr=1e-4))          # (a reference checkpoint: no optimizer state)
    assert got["epoch"] == 3 and all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), net.state_dict().values()))
    fit.load_model_state(other, ck["model_state_dict"])                                          # and without the prefix
    with pytest.raises(KeyError, match="model_state_dict"):
        fit.load_checkpoint({"epoch": 1}, other)
    with pytest.raises(RuntimeError):
        fit.load_model_state(other, {"module." + k: v for k, v in list(ck["model_state_dict"].items())[:1]})


def test_clip_sets_follow_the_parameter_names():
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.RNet, self.SNet, self.head = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    net = Net()
    r, s = fit.clip_sets(net)
    assert [id(p) for p in r] == [id(p) for p in net.RNet.parameters()] and [id(p) for p in s] == [id(p) for p in net.SNet.parameters()]
