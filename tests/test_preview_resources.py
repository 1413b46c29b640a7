"""Register / scratch gate of the preview unit (csrc/preview.hip): no kernel of it may touch scratch memory or spill a register.  Same
source of numbers and same parser as tests/test_kernel_resources.py."""
from test_kernel_resources import _remarks, _table

KERNELS = {"preview_range_kernel", "preview_grid_kernel", "kernel_from_kinfo_kernel"}


def test_preview_kernels_do_not_use_scratch():
    rows = _table(_remarks("preview"))
    assert rows, "no kernel-resource remarks for preview"
    names = {r["pretty"].replace("void ", "") for r in rows}
    assert KERNELS <= names, names
    bad = [(r["pretty"], r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for r in rows
           if r.get("ScratchSize [bytes/lane]", 0) != 0 or r.get("VGPRs Spill", 0) != 0]
    assert not bad, f"preview: kernels that use scratch (name, bytes/lane, spilled VGPRs): {bad}"
