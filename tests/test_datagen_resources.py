"""Register / scratch gate of the batch-synthesis unit (csrc/datagen.hip): no kernel of it may touch scratch memory.  Same source of numbers
and same parser as tests/test_kernel_resources.py."""
from test_kernel_resources import _remarks, _table

KERNELS = {"datagen_patch_kernel<0>", "datagen_patch_kernel<1>", "datagen_patch_kernel<2>", "datagen_normal_kernel", "datagen_blur_kernel"}


def test_datagen_kernels_do_not_use_scratch():
    rows = _table(_remarks("datagen"))
    assert rows, "no kernel-resource remarks for datagen"
    names = {r["pretty"].replace("void ", "") for r in rows}
    assert KERNELS <= names, names
    bad = [(r["pretty"], r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for r in rows
           if r.get("ScratchSize [bytes/lane]", 0) != 0 or r.get("VGPRs Spill", 0) != 0]
    assert not bad, f"datagen: kernels that use scratch (name, bytes/lane, spilled VGPRs): {bad}"
