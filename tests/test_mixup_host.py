"""Host-side checks of the device MixUp and the real-noise batch (virnet_amd/datagen.py, csrc/datagen.hip): the C entries are bound at ABI
version 5, the numpy definition is the reference's ``MixUp_AUG.aug`` bit for bit (tests/golden/mixup.npz, made by
tests/golden/make_mixup_golden.py), the drawer consumes torch's global generator as the reference does, and argument errors are raised
before any device work."""
import os
import re

import numpy as np
import pytest
import torch

import datagen_cases as dc
import mixup_cases as mc
from conftest import REPO, load_golden
from virnet_amd import _native, datagen

NEW_SYMBOLS = ("virnet_mixup", "virnet_datagen_pair_mix")


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
        assert re.search(r"\bint\s+%s\(" % name, header)


def test_the_definition_is_the_reference_bit_for_bit():
    G = load_golden("mixup")
    mix = datagen.MixParams(G["perm"], G["lam"])
    assert G["gt"].shape == (9, 3, 20, 20) and G["gt"].dtype == np.float32
    assert dc.same_bits(datagen.mixup_np(G["gt"], mix), G["out_gt"])
    assert dc.same_bits(datagen.mixup_np(G["noisy"], mix), G["out_noisy"])
    # the bar discriminates: one rounding instead of three (what a contracted multiply-add gives) is another result
    lam = G["lam"].astype(np.float64).reshape(-1, 1, 1, 1)
    fused = (lam * G["gt"] + (1.0 - lam) * G["gt"][G["perm"]]).astype(np.float32)
    assert not dc.same_bits(fused, G["out_gt"])


def test_the_drawer_consumes_the_global_generator_as_the_reference_does():
    G = load_golden("mixup")
    torch.manual_seed(int(G["seed"]))
    mix = datagen.draw_mixup_params(9)
    assert np.array_equal(mix.perm, G["perm"]) and dc.same_bits(mix.lam, G["lam"])
    for n, seed, alpha in ((9, 3, 0.6), (16, 1234, 0.6), (1, 5, 0.6), (7, 8, 1.5)):
        torch.manual_seed(seed)
        perm = torch.randperm(n)
        lam = torch.distributions.beta.Beta(torch.tensor([alpha]), torch.tensor([alpha])).rsample((n, 1))
        after = torch.rand(1)
        torch.manual_seed(seed)
        mix = datagen.draw_mixup_params(n, alpha)
        assert torch.equal(torch.rand(1), after)           # the generator is left in the same state
        assert mix.n == n and mix.perm.dtype == np.int32 and mix.lam.dtype == np.float32
        assert np.array_equal(mix.perm, perm.numpy()) and dc.same_bits(mix.lam, lam.reshape(-1).numpy())
        assert sorted(mix.perm.tolist()) == list(range(n))


def test_the_ends_of_the_range_return_the_sample_and_the_partner():
    a, _ = mc.tensors((9, 3, 20, 20))
    perm = np.asarray(mc.PERM)
    assert dc.same_bits(datagen.mixup_np(a, datagen.MixParams(perm, np.ones(9))), a)
    assert dc.same_bits(datagen.mixup_np(a, datagen.MixParams(perm, np.zeros(9))), a[perm])
    got = datagen.mixup_np(a, mc.mix())
    assert dc.same_bits(got[2], a[2]) and dc.same_bits(got[1], a[2]) and dc.same_bits(got[0], a[0])      # lam 1, lam 0, the fixed point at 1/2


@pytest.mark.parametrize("perm, lam, word", [([0, 1, 3], [0.5, 0.5, 0.5], "perm"), ([0, -1, 2], [0.5, 0.5, 0.5], "perm"),
                                             ([0, 1, 2], [0.5, float("nan"), 0.5], "lam"), ([0, 1, 2], [0.5, 1.5, 0.5], "lam"),
                                             ([0, 1, 2], [0.5, -1e-3, 0.5], "lam"), ([0, 1, 2], [0.5, float("inf"), 0.5], "lam"),
                                             ([0, 1, 2], [0.5, 0.5], "perm has 3 entries but lam has 2"), ([], [], "perm")],
                         ids=["index_n", "negative_index", "nan", "above_one", "below_zero", "inf", "lengths", "empty"])
def test_validate_refuses_by_name(perm, lam, word):
    with pytest.raises(ValueError, match=word):
        datagen.MixParams(np.asarray(perm, dtype=np.int64), lam)
    with pytest.raises(TypeError, match="perm"):
        datagen.MixParams([0.0, 1.0], [0.5, 0.5])
    assert datagen.MixParams([1, 1, 0], [0.0, 1.0, 0.25]).n == 3          # a repeated index is accepted


def test_pack_layout():
    mix = mc.mix()
    blob = mix.pack()
    assert blob.dtype == np.uint8 and blob.shape == (8 * 9,)
    assert np.array_equal(blob[:36].view(np.int32), np.asarray(mc.PERM, dtype=np.int32))
    assert dc.same_bits(blob[36:].view(np.float32), mc.LAM)


class _NoLaunch:
    """stands in for the loaded library: any call into it is an error"""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: argument errors must be raised before any device work")


@pytest.fixture
def no_device_work(monkeypatch):
    monkeypatch.setattr(datagen._native, "load", lambda: _NoLaunch())
    return datagen


@pytest.mark.parametrize("case, exc", [("cpu", RuntimeError), ("shape", ValueError), ("fp16", TypeError), ("mix_n", ValueError), ("dims", ValueError),
                                       ("mix_type", TypeError)])
def test_mixup_argument_errors_before_device_work(no_device_work, case, exc):
    a, b, mix = torch.zeros(9, 3, 20, 20), torch.zeros(9, 3, 20, 20), mc.mix()
    if case == "shape":
        b = torch.zeros(9, 3, 20, 24)
    elif case == "fp16":
        a = a.half()
    elif case == "mix_n":
        mix = mc.mix_for(5)
    elif case == "dims":
        a, b = a[0], b[0]
    elif case == "mix_type":
        mix = (mc.PERM, mc.LAM)
    with pytest.raises(exc) as e:
        no_device_work.mixup(a, b, mix)
    if case == "cpu":
        assert "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("case, exc", [("cpu", RuntimeError), ("unpaired", ValueError), ("mix_n", ValueError), ("k_even", ValueError),
                                       ("k_pad", ValueError), ("k_large", ValueError), ("patch", ValueError), ("mix_type", TypeError)])
def test_real_batch_argument_errors_before_device_work(no_device_work, case, exc):
    p, mix, k = 20, mc.mix(), 7
    ims, other = list(dc.images(0)), list(dc.images(1))
    pool = datagen.ImagePool(ims, "cpu") if case == "unpaired" else datagen.ImagePool.paired(ims, other, "cpu")
    params = dc.params(p)
    if case == "mix_n":
        mix = mc.mix_for(5)
    elif case == "k_even":
        k = 6
    elif case == "k_pad":
        p, k = 3, 7                                       # k // 2 = 3 is not < 3
        params = datagen.BatchParams(dc.SHAPES, 3, [0] * 9, [0] * 9, [0] * 9, dc.FLAGS)
    elif case == "k_large":
        k = 33
    elif case == "patch":
        p = 33
    elif case == "mix_type":
        mix = None
    with pytest.raises(exc) as e:
        no_device_work.real_batch(pool, params, p, mix, k)
    if case == "cpu":
        assert "no CPU fallback" in str(e.value)


def test_c_abi_argument_errors_return_nonzero_with_a_message():
    """bad arguments never reach a launch: the entries return non-zero and set virnet_last_error (no device needed, pointers are never read)"""
    lib = _native.load()
    a, b, mix, oa, ob = (k << 20 for k in range(1, 6))      # non-NULL, 16-byte aligned, 1 MiB apart: rejected calls do not touch them

    def err():
        return lib.virnet_last_error().decode()
    for i in range(5):
        ptrs = [a, b, mix, oa, ob]
        ptrs[i] = 0
        assert lib.virnet_mixup(*ptrs, 2, 64, None) != 0 and "NULL" in err()
        ptrs[i] = [a, b, mix, oa, ob][i] + 2
        assert lib.virnet_mixup(*ptrs, 2, 64, None) != 0 and "misaligned" in err()
    for n in (0, -1, 65536):
        assert lib.virnet_mixup(a, b, mix, oa, ob, n, 64, None) != 0 and "samples" in err()
    for per in (0, -4, 1 << 31):
        assert lib.virnet_mixup(a, b, mix, oa, ob, 2, per, None) != 0 and "elements per sample" in err()
    # in place, an output inside an input's range, an input starting inside an output, the two outputs on each other, an output on the mix
    for ptrs in ((a, b, mix, a, ob), (a, b, mix, oa, b), (a, b, mix, a + 256, ob), (oa + 256, b, mix, oa, ob), (a, b, mix, oa, oa + 508),
                 (a, b, mix, oa, mix - 508), (a, b, mix, mix + 12, ob)):
        assert lib.virnet_mixup(*ptrs, 2, 64, None) != 0 and "overlap" in err()

    pa, pb, table, params, mx, o0, o1 = (k << 20 for k in range(1, 8))
    good = [pa, pb, table, params, mx, 2, 20, o0, o1]
    for i in (0, 1, 2, 3, 4, 7, 8):
        args = list(good)
        args[i] = 0
        assert lib.virnet_datagen_pair_mix(*args, None) != 0 and "NULL" in err()
        if i >= 2:
            args[i] = good[i] + 2
            assert lib.virnet_datagen_pair_mix(*args, None) != 0 and "aligned" in err()
    for n in (0, 65536):
        assert lib.virnet_datagen_pair_mix(pa, pb, table, params, mx, n, 20, o0, o1, None) != 0 and "samples" in err()
    for p in (0, datagen.MAX_PATCH + 1):
        assert lib.virnet_datagen_pair_mix(pa, pb, table, params, mx, 2, p, o0, o1, None) != 0 and "patch size" in err()
    size = 2 * 3 * 20 * 20 * 4
    for args in ((pa, pb, table, params, mx, 2, 20, o0, o0), (pa, pb, table, params, mx, 2, 20, o0, o0 + size - 4), (pa, pb, table, o0 + 8, mx, 2, 20, o0, o1),
                 (pa, pb, table, params, o1 - 12, 2, 20, o0, o1), (o0 + 100, pb, table, params, mx, 2, 20, o0, o1), (pa, o1, table, params, mx, 2, 20, o0, o1),
                 (pa, pb, o0 + 64, params, mx, 2, 20, o0, o1)):
        assert lib.virnet_datagen_pair_mix(*args, None) != 0 and "overlap" in err()
    # the existing entry keeps refusing modes outside 0..2
    assert lib.virnet_datagen_patches(3, pa, pb, table, params, 2, 20, None, None, 0, 0, 0, o0, o1, None, None) != 0 and "mode" in err()
