"""Register / scratch gate of the weight-average unit (csrc/ema.hip): no kernel of it may touch scratch memory or spill a register.  Same
source of numbers and same parser as tests/test_kernel_resources.py."""
from test_kernel_resources import _remarks, _table

KERNELS = {"ema_kernel<0>", "ema_kernel<1>"}


def test_ema_kernels_do_not_use_scratch():
    rows = _table(_remarks("ema"))
    assert rows, "no kernel-resource remarks for ema"
    names = {r["pretty"].replace("void ", "") for r in rows}
    assert KERNELS <= names, names
    bad = [(r["pretty"], r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for r in rows
           if r.get("ScratchSize [bytes/lane]", 0) != 0 or r.get("VGPRs Spill", 0) != 0]
    assert not bad, f"ema: kernels that use scratch (name, bytes/lane, spilled VGPRs): {bad}"
