"""Host-side checks of the composed tail: the register / scratch budget of the exit kernel's additive-map instantiations (the
compiler's own numbers, read as tests/test_kernel_resources.py reads them), the symbols, and the conditions under which
engine._tail_composition leaves the two launches alone without touching a device."""
import re

import torch

from virnet_amd import _native, engine
from virnet_amd.networks.AttResUNet import AttResUNet
from test_kernel_resources import _remarks, _table


def test_additive_exit_kernels_use_no_scratch_and_spill_nothing():
    rows = [r for r in _table(_remarks("conv_exit")) if "conv_exit_zadd_kernel" in r["pretty"]]
    assert sorted(re.search(r"conv_exit_zadd_kernel<\d>", r["pretty"]).group(0) for r in rows) == ["conv_exit_zadd_kernel<4>", "conv_exit_zadd_kernel<6>"], rows
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 256, r            # two waves per SIMD, as the plain kernels (190 / 142 registers)


def test_symbols_bound_and_abi_version_unchanged():
    names = {s[0] for s in _native.SYMBOLS}
    assert {"virnet_conv_exit_add", "virnet_compose_exit_weight"} <= names
    assert _native.ABI_VERSION == 5


def test_composition_is_off_in_grad_mode_fp32_forms_and_by_the_knob(monkeypatch):
    for k in ("VIRNET_CONV_FORM", "VIRNET_WINOGRAD", "VIRNET_TAIL_COMPOSE", "VIRNET_EXIT_FORM"):
        monkeypatch.delenv(k, raising=False)
    rnet = AttResUNet(in_chn=3, extra_chn=1, out_chn=3, n_resblocks=1, n_feat=[96, 192], extra_mode="Input")
    with torch.enable_grad():
        assert engine._tail_composition(rnet) is None
    with torch.no_grad():
        for k, v in (("VIRNET_TAIL_COMPOSE", "0"), ("VIRNET_EXIT_FORM", "f16"), ("VIRNET_CONV_FORM", "wino"), ("VIRNET_CONV_FORM", "direct")):
            monkeypatch.setenv(k, v)
            assert engine._tail_composition(rnet) is None, (k, v)
            monkeypatch.delenv(k)
        assert engine._tail_composition(AttResUNet(in_chn=3, extra_chn=1, out_chn=3, n_resblocks=1, n_feat=[96], extra_mode="Input")) is None
        assert engine._tail_composition(AttResUNet(in_chn=3, extra_chn=1, out_chn=3, n_resblocks=1, n_feat=[128, 192], extra_mode="Input")) is None
    assert len(rnet._cache.slots()) == 0
