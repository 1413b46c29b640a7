"""The preview kernels under the software red zone (tests/redzone.py), at the ragged shapes of tests/test_preview_gpu.py: inputs in guarded
arenas (also as views at odd element offsets, and as three channels of a four-channel batch whose fourth channel is NaN), the workspace
and the event buffer from the package's own ``torch.empty`` inside the guard.  Nothing may be written outside a buffer, no zone or
unwritten word may reach a result, and every byte of every grid must be written -- the byte ends of a grid that starts at an odd address
included."""
import numpy as np
import pytest
import torch

from redzone import guarded
from virnet_amd import preview as pv

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 5, 7), (9, 1, 21, 21), (3, 1, 6, 5), (2, 3, 33, 31), (8, 3, 16, 16)]


def _values(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("skew", [0, 1, 3])
def test_grids_stay_inside_their_buffers(skew):
    with guarded() as g:
        xs, specs = [], []
        for i, shape in enumerate(SHAPES):
            x_np = _values(shape, i)
            flat = g.input(torch.from_numpy(np.concatenate([np.zeros(skew, np.float32), x_np.reshape(-1)])).cuda())
            xs.append(x_np)
            specs.append(dict(x=flat[skew:].view(shape), clamp=(-1.0, 1.0) if i % 2 else None))
        n_before = len(g.arenas)
        grids = pv.grids(specs)
        assert len(g.arenas) == n_before + 1 + len(SHAPES)                         # the event buffer and one workspace per grid, all guarded
        g.check(grids)
        assert any(t.data_ptr() % 4 for t in grids)                                # some grid starts between two dwords
        for t, x_np, s in zip(grids, xs, specs):
            assert np.array_equal(t.cpu().numpy(), pv.grid_np(x_np, clamp=s["clamp"]))
        # a lone grid: its own buffer
        one = pv.grid(specs[3]["x"], nrow=1, padding=3)
        g.check([one])
        assert np.array_equal(one.cpu().numpy(), pv.grid_np(xs[3], nrow=1, padding=3))


def test_three_channels_of_four_do_not_read_the_fourth():
    with guarded() as g:
        x_np = _values((5, 4, 9, 11), 9)
        x_np[:, 3] = np.nan                                                         # read by mistake, it would empty every range
        x = g.input(torch.from_numpy(x_np).cuda())
        out = pv.grid(x, channels=3)
        g.check([out])
        want = pv.grid_np(np.ascontiguousarray(x_np[:, :3]))
        assert np.array_equal(out.cpu().numpy(), want) and want.max() == 255
        last = pv.grid(x[4:5], channels=3)                                          # the last image: right in front of the back zone
        g.check([last])
        assert np.array_equal(last.cpu().numpy(), pv.grid_np(np.ascontiguousarray(x_np[4:5, :3])))


@pytest.mark.parametrize("k,n", [(21, 5), (15, 1), (25, 3), (1, 2)])
def test_kernel_from_kinfo_stays_inside_its_buffers(k, n):
    with guarded() as g:
        r = np.random.default_rng(k)
        info = np.concatenate([r.uniform(0.5, 12.0, (n, 2)), r.uniform(-0.9, 0.9, (n, 1))], axis=1).astype(np.float32)
        dev = g.input(torch.from_numpy(info).cuda())
        n_before = len(g.arenas)
        out = pv.kernel_from_kinfo(dev, k, 2, True)
        assert len(g.arenas) == n_before + 1                                        # the result only: no workspace
        g.check([out])
        got, want = out.cpu().numpy(), pv.kernel_np(info, k, 2, True)
        assert np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() <= 1
