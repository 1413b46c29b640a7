"""CPU tests of the one-product fp16 Winograd form (VIRNET_CONV_FORM=wx4x1; csrc/conv_f16_wx4x1.hip): the ABI, the form rule, the launch
plans, the numerics gate's ordering of the reduced-precision arithmetics, the inputs of the GPU tests, and the kernels' resources."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch
import torch.nn.functional as F

import wx4x1_ref
from virnet_amd import _native, ops
from test_conv_form import KNOBS, rule_of, table
from test_kernel_resources import _remarks, _table
from test_launch_plan import desc_of
from test_ops_gpu import make_conv, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_declared_and_bound_and_the_abi_is_5():
    lib = _native.load()
    assert lib.virnet_abi_version() == 5 == _native.ABI_VERSION
    fn = lib.virnet_conv_wx4x1
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 2
    with open(os.path.join(ROOT, "include", "virnet_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int virnet_conv_wx4x1\(const virnet_conv_desc\* d, void\* stream\);", header, re.M)
    assert "#define VIRNET_ABI_VERSION 5" in header
    assert re.search(r"VIRNET_PLAN_WX4X1 = %d\b" % _native.PLAN_WX4X1, header)
    assert ops._CONV_FORMS["wx4x1"] == ("virnet_conv_wx4x1", "wx4", "conv_wx4x1") and "wx4x1" in ops._F16_FAMILY
    assert lib.virnet_conv_wx4x1(None, None) != 0 and b"desc is NULL" in lib.virnet_last_error()


def test_form_value_packs_the_wx4_image_and_keeps_the_guard(monkeypatch):
    monkeypatch.setenv("VIRNET_CONV_FORM", "wx4x1")
    assert ops.conv_form() == "wx4x1" and ops._f16_family()
    monkeypatch.setenv("VIRNET_CONV_FORM", "wx4")
    want = {k: ops.pack_images_rule(*k) for k in [("conv", 1, 3, 96, 96), ("conv", 1, 3, 3, 96), ("conv", 2, 3, 96, 192), ("convt", 2, 2, 192, 96),
                                                  ("conv", 1, 3, 96, 3), ("conv", 1, 3, 64, 64)]}
    monkeypatch.setenv("VIRNET_CONV_FORM", "wx4x1")
    assert {k: ops.pack_images_rule(*k) for k in want} == want
    monkeypatch.setenv("VIRNET_CONV_FORM", "wx4x2")
    with pytest.raises(ValueError, match="wx4x1"):
        ops.conv_form()


def test_rule_is_the_wx4_rule_with_the_form_renamed():
    """Every spec row of tests/golden/conv_forms.json (rows that ask for an emission excluded) under each of its knob sets: where
    VIRNET_CONV_FORM=wx4 gives wx4, wx4x1 gives wx4x1; everywhere else the two agree."""
    tab = table()
    layers = {k: tuple(v[f] for f in ("transposed", "stride", "c", "cout", "cstore")) for k, v in tab["layers"].items()}
    before = {k: os.environ.get(k) for k in KNOBS}
    seen = {"renamed": 0, "same": 0}
    try:
        for row in tab["rows"]:
            if row[7] != 0:
                continue
            got = {}
            for form in ("wx4", "wx4x1"):
                r = list(row)
                r[8] = dict(row[8], VIRNET_CONV_FORM=form)
                got[form] = rule_of(r, layers[row[0]], os.environ)
            if got["wx4"][0] == "wx4":
                assert got["wx4x1"] == ("wx4x1", 0), (row[:9], got)
                seen["renamed"] += 1
            else:
                assert got["wx4x1"] == got["wx4"], (row[:9], got)
                seen["same"] += 1
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert seen["renamed"] > 100 and seen["same"] > 100, seen


@pytest.mark.parametrize("c", [64, 96, 160, 192, 224, 288])
@pytest.mark.parametrize("n,h,w", [(1, 3, 2), (1, 17, 70), (32, 256, 256)])
def test_plan_covers_every_slab_exactly_once(monkeypatch, c, n, h, w):
    for k in ("VIRNET_WX4_NREP", "VIRNET_WX4_ROWS", "VIRNET_DETERMINISTIC", "VIRNET_WX4_MIN_WGS"):
        monkeypatch.delenv(k, raising=False)
    d = desc_of([_native.PLAN_WX4X1, n, h, w, c, c, 1, 0, 1, 1, 0, 256])
    for pin in (None, "1", "2", "3"):
        if pin:
            monkeypatch.setenv("VIRNET_WX4_NREP", pin)
        plan = ops.conv_plan_query(_native.PLAN_WX4X1, d, n_cu=256)
        slabs = [s for l in plan for s in range(l["slab_base"], l["slab_base"] + l["groups"] * l["ng"] * l["nrep"])]
        assert slabs == list(range(c // 32)), (pin, plan)
        assert all(l["form"] == 6 and l["rows"] == 16 and l["ng"] == 1 and 1 <= l["nrep"] <= 3 and not l["persistent"] for l in plan), plan
        if pin is None and n == 32:                          # the chip is full: three slabs per workgroup, the remainder in twos
            assert [l["nrep"] for l in plan] == {2: [2], 3: [3], 5: [3, 2], 6: [3], 7: [3, 2], 9: [3]}[c // 32], plan
        if pin is None and n == 1:                           # CUs left empty: one slab per workgroup, one launch
            assert [l["nrep"] for l in plan] == [1], plan
    with pytest.raises(RuntimeError, match="emit_rows"):
        ops.conv_plan_query(_native.PLAN_WX4X1, d, emit_rows=16, n_cu=256)


def _gate():
    spec = importlib.util.spec_from_file_location("numerics_gate", os.path.join(ROOT, "tools", "numerics_gate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gate_orders_the_reduced_precision_arithmetics():
    """Whole denoise-syn network at 48^2 against fp64: one fp16 Winograd product is better than the bf16 form's arithmetic, one bf16
    Winograd product is worse (so nobody builds it)."""
    rows, _, _, _ = _gate().gate(48, 1, ["wx4x1", "bf16x1", "wx4_b1"])
    r = {x["mode"]: x for x in rows}
    for k in ("mu_max_abs", "mu_rms", "sigma_max_rel"):
        assert 0 < r["wx4x1"][k] < r["bf16x1"][k] < r["wx4_b1"][k], (k, r)


def test_emulation_matches_a_float64_winograd_and_the_weight_image_rule():
    """tests/wx4x1_ref.py against itself: without the two fp16 rounds the same code is an fp32-class convolution, and the weight operand is
    the scaled transform to half an fp16 ulp with row maxima in [8192, 16384)."""
    cp = make_conv(64, 64, seed=3)
    w = cp.weight.detach().clone()
    w[5] *= 1e-3
    us, inv = wx4x1_ref.weight_operand(w)
    u = torch.einsum("jb,okdb->okdj", wx4x1_ref.G, w.double())
    assert torch.all(torch.log2(inv) == torch.log2(inv).round())
    smax = u.abs().amax(dim=(1, 2, 3)) / inv.double()
    assert torch.all((smax >= 8192) & (smax < 16384))
    assert float((us * inv.double().view(-1, 1, 1, 1) - u).abs().max() / u.abs().max()) <= 2.0 ** -11
    x = rnd(1, 64, 7, 13, seed=4)
    v = wx4x1_ref.input_transform(x).double()
    y = sum(torch.einsum("ocj,nchtj->nohtj", u[:, :, dy, :], v[:, :, dy:dy + 7]) for dy in range(3))
    y = torch.einsum("kj,nohtj->nohtk", wx4x1_ref.AT.double(), y).reshape(1, 64, 7, -1)[..., :13]
    assert float((y - F.conv2d(x.double(), w.double(), padding=1)).abs().max()) <= 2e-5


@pytest.mark.parametrize("c,h,w,n", wx4x1_ref.SHAPES)
def test_gpu_test_inputs_leave_room_below_bf16(c, h, w, n):
    """The inputs of tests/test_conv_wx4x1_gpu.py's layer cases: the emulation's error is at most 0.7 of the bf16-operand conv's, so the
    GPU bars B (e_k <= 1.5 e_m) and C (e_k < e_b) do not contradict each other."""
    cp = make_conv(c, c, seed=80)
    x, res = rnd(n, c, h, w, seed=81), rnd(n, c, h, w, seed=82)
    _, _, e_m, e_b = wx4x1_ref.three_errors(F.leaky_relu(x, 0.2), cp.weight.detach(), cp.bias.detach(), lambda y: y + res.to(y.dtype))
    print(f"c{c} {n}x{h}x{w}: e_m {e_m:.3e}  e_b {e_b:.3e}  ratio {e_m / e_b:.3f}")
    assert 0 < e_m <= 0.7 * e_b, (e_m, e_b)


def test_new_unit_uses_no_scratch():
    rows = _table(_remarks("conv_f16_wx4x1"))
    kernels = [r for r in rows if "conv_wx4x1_kernel" in r["pretty"]]
    assert len(kernels) == 45, len(kernels)                   # 3 slab counts x 5 epilogues x 3 pre-activations
    for r in rows:
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r
