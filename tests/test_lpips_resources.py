"""Register / scratch gate of the LPIPS unit (csrc/lpips.hip): the exact set of its kernels, none of which may touch scratch memory or spill
a vector register.  Same source of numbers and same parser as tests/test_kernel_resources.py."""
from test_kernel_resources import _remarks, _table

KERNELS = {"lpips_stem_kernel", "lpips_pool_kernel", "lpips_conv_kernel<5>", "lpips_conv_kernel<3>", "lpips_score_kernel",
           "lpips_finish_kernel", "lpips_nchw_kernel"}


def test_lpips_kernels_do_not_use_scratch():
    rows = _table(_remarks("lpips"))
    assert rows, "no kernel-resource remarks for lpips"
    names = {r["pretty"].replace("void ", "") for r in rows}
    assert KERNELS == names, names
    bad = [(r["pretty"], r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for r in rows
           if r.get("ScratchSize [bytes/lane]", 0) != 0 or r.get("VGPRs Spill", 0) != 0]
    assert not bad, f"lpips: kernels that use scratch (name, bytes/lane, spilled VGPRs): {bad}"
