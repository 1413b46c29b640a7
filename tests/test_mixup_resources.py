"""Register / scratch gate of the MixUp kernels (csrc/datagen.hip): both must be in the compiler's resource remarks with zero scratch and no
spilled vector register.  Same source of numbers and same parser as tests/test_datagen_resources.py."""
from test_kernel_resources import _remarks, _table

KERNELS = {"mixup_kernel", "datagen_pair_mix_kernel"}


def test_mixup_kernels_do_not_use_scratch():
    rows = [r for r in _table(_remarks("datagen")) if r["pretty"].replace("void ", "") in KERNELS]
    assert {r["pretty"].replace("void ", "") for r in rows} == KERNELS, [r["pretty"] for r in rows]
    for r in rows:
        assert "ScratchSize [bytes/lane]" in r and "VGPRs Spill" in r, r
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r
