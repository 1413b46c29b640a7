"""The pinned instantiations of the fp32 direct convolution under the software red zone (tests/redzone.py): the rows mfma_cases.REDZONE
names -- per (KS, STRIDE, MREP, NW) the largest and the smallest NREP, and the planar rows with 5 and with 32 channels, whose `n >= cout`
skip and crop are all that keeps their stores inside the buffer.  tests/test_redzone_gpu.py runs this kernel at shapes where every
launch is <KS, STRIDE, 1, 1>; here the input, the weight, its packed image, the per-image vectors and the outputs of a multi-slab, an
eight-row and an eight-wave launch sit between guard zones, with the last image's partial tile next to the zone: no zone is written,
every result element is written, none is NaN, and the guarded result has the bits of the unguarded one."""
import ctypes

import pytest

from mfma_cases import BY_ID, REDZONE
from test_conv_mfma_gpu import Case, setenv
from test_redzone_gpu import run_guarded
from virnet_amd import _native as nat

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rid", REDZONE)
def test_pinned_instantiation_stays_inside_its_buffers(monkeypatch, rid):
    row = BY_ID[rid]
    setenv(monkeypatch, row.env)
    case = Case(row)
    _, rec = run_guarded(case.call, case.tensors, [case.cp], names=["direct"])
    assert [k for k in rec.timer.summary() if isinstance(k[0], int)] == [row.tile[:4]]
    tiles = []
    for d, form, _ in rec.convs:                               # (the tile rule reads the descriptor's extents, no pointer)
        v = (ctypes.c_int * 5)()
        nat.check(nat.load().virnet_conv_mfma_tile(ctypes.byref(d), ctypes.byref(v)), "conv_mfma_tile")
        tiles.append((form, tuple(v)))
    assert tiles == [("direct", row.tile)], tiles
