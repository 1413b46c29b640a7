"""The LPIPS kernels under the software red zone (tests/redzone.py) at the minimum size, the partly padded last window and the multi-tile
case: images enter through ``g.input``; the packed weights, the workspace and the results come from the package's own ``torch.empty``
inside the guard, so every buffer a kernel touches has zones on both sides.  Nothing may be written outside a buffer, every result
element must be written, and no guard-zone or unwritten NaN may reach a result (the workspace's rounding gaps are never read).  A stray
read of a uint8 image cannot show up as NaN; the comparison with the fp64 definition catches it by value."""
import pytest
import torch

import lpips_cases as lc
from redzone import guarded
from test_lpips_gpu import DIST_REL, TAP_REL
from virnet_amd import lpips

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", lc.FORMS)
@pytest.mark.parametrize("case", lc.EDGE_CASES, ids=lc.EDGE_IDS)
def test_distance_and_features_stay_inside_their_buffers(case, form):
    a, b = lc.pair(case, form)
    want_d, want_taps = lc.reference(case, form)
    w = lpips.synth_weights(lc.SEED)                        # a fresh object: its device copies are made inside the guard
    with guarded() as g:
        da, db = g.input(a.cuda()), g.input(b.cuda())
        got = lpips.distance(da, db, w)
        taps = lpips.features(da, w)
        g.check([got, taps])
        workspaces = [ar for ar in g.arenas if ar.dtype == torch.int64]
        assert len(workspaces) == 2                         # one per call, each with its own zones (checked above and on leaving)
        assert len([ar for ar in g.arenas if ar.dtype == torch.float32 and ar.shape == (363, 64)]) == 1      # the packed conv1 weight
        assert float(((got.cpu() - want_d).abs() / want_d).max()) <= DIST_REL
        for t, r, bar in zip(taps, want_taps, TAP_REL):
            assert float((t.cpu().double() - r).abs().max() / r.abs().max()) <= bar
