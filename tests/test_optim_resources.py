"""Register / scratch gate of the optimizer unit (csrc/optim.hip): no kernel of it may touch scratch memory.  Same source of numbers and same
parser as tests/test_kernel_resources.py."""
from test_kernel_resources import _remarks, _table

KERNELS = {"optim_sqnorm_kernel", "optim_finish_kernel", "optim_apply_kernel<0>", "optim_apply_kernel<1>", "optim_apply_kernel<2>"}


def test_optim_kernels_do_not_use_scratch():
    rows = _table(_remarks("optim"))
    assert rows, "no kernel-resource remarks for optim"
    names = {r["pretty"].replace("void ", "") for r in rows}
    assert KERNELS <= names, names
    bad = [(r["pretty"], r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for r in rows
           if r.get("ScratchSize [bytes/lane]", 0) != 0 or r.get("VGPRs Spill", 0) != 0]
    assert not bad, f"optim: kernels that use scratch (name, bytes/lane, spilled VGPRs): {bad}"
