"""Register / scratch gate of the self-ensemble unit (csrc/ensemble.hip): no kernel of it may touch scratch memory.  Same source of numbers
and same parser as tests/test_kernel_resources.py."""
from test_kernel_resources import _remarks, _table

KERNELS = {"ensemble_expand_kernel<unsigned char>", "ensemble_expand_kernel<float>",
           "ensemble_reduce_kernel<unsigned char, 0>", "ensemble_reduce_kernel<unsigned char, 1>",
           "ensemble_reduce_kernel<float, 0>", "ensemble_reduce_kernel<float, 1>"}


def test_ensemble_kernels_do_not_use_scratch():
    rows = _table(_remarks("ensemble"))
    assert rows, "no kernel-resource remarks for ensemble"
    names = {r["pretty"].replace("void ", "") for r in rows}
    assert KERNELS == names, names                                  # two kernel families and no others
    bad = [(r["pretty"], r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for r in rows
           if r.get("ScratchSize [bytes/lane]", 0) != 0 or r.get("VGPRs Spill", 0) != 0]
    assert not bad, f"ensemble: kernels that use scratch (name, bytes/lane, spilled VGPRs): {bad}"
