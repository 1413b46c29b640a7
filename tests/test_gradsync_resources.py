"""Register / scratch gate of the gradient-bucket unit (csrc/gradsync.hip): its kernel may not touch scratch memory.  Same source of numbers
and same parser as tests/test_kernel_resources.py."""
from test_kernel_resources import _remarks, _table

KERNELS = {"gradsync_copy_kernel"}


def test_gradsync_kernels_do_not_use_scratch():
    rows = _table(_remarks("gradsync"))
    assert rows, "no kernel-resource remarks for gradsync"
    names = {r["pretty"].replace("void ", "") for r in rows}
    assert KERNELS <= names, names
    bad = [(r["pretty"], r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for r in rows
           if r.get("ScratchSize [bytes/lane]", 0) != 0 or r.get("VGPRs Spill", 0) != 0]
    assert not bad, f"gradsync: kernels that use scratch (name, bytes/lane, spilled VGPRs): {bad}"
