"""The weight average on the GPU (virnet_amd/ema.py, csrc/ema.hip) on the tensor set of tests/ema_cases.py: the update against the numpy
definition bit for bit, with warm-up over three steps, next to the view parameter's neighbours, with NaN / Inf in place and twice from
one start; the swap as an exact exchange that bumps ``_version``; a network under automatic graph replay running on the averaged weights
and back; the update after a ``torch.optim.Adam`` step; and the absence of host synchronisation."""
import numpy as np
import pytest
import torch

import ema_cases as ec
from virnet_amd import graph
from virnet_amd.ema import WeightEMA, weight_at
from virnet_amd.networks import VIRAttResUNet
from virnet_amd.utils.synth import synth_images, synth_state_dict

pytestmark = pytest.mark.gpu
DECAY = 0.999


def _run_once():
    ema, params, buf = ec.make_ema("cuda", decay=DECAY)
    ema.update()
    return ema, params, buf


@pytest.fixture(scope="module")
def one_update():
    """one update of the whole set from values(0): shared (read-only) by the tests below, with its reference"""
    ema, params, buf = _run_once()
    ps, es = ec.values(0)
    return dict(ema=ema, params=params, buf=buf, want=ec.reference_update(es, ps, weight_at(0, DECAY)))


def test_one_update_is_the_numpy_definition_bit_for_bit(one_update):
    ema = one_update["ema"]
    assert ema.num_updates == 1 and not ema.swapped and len(ema.shadows) == len(ec.ALL_SIZES) > ec.TABLE
    assert ema.shadows[ec.I_VIEW].data_ptr() % 16 == 0 and ema.params[ec.I_VIEW].data_ptr() % 16 == 4          # the pair takes the 4-byte form
    ec.assert_same(ema.shadows, one_update["want"], "update")
    ps, es = ec.values(0)
    for i, (s, e, p) in enumerate(zip(ema.shadows, es, one_update["params"])):
        mask = ec.fixpoints(i).numpy()
        assert np.array_equal(ec.bits(s)[mask], ec.bits(e)[mask])                  # p == e: bitwise unchanged
        assert np.array_equal(ec.bits(p), ec.bits(ps[i]))                          # the parameters are read only
        if mask.sum() < mask.size - 3:
            assert not np.array_equal(ec.bits(s)[~mask], ec.bits(e)[~mask])


def test_the_view_buffers_neighbours_are_untouched(one_update):
    buf = one_update["buf"].cpu()
    assert float(buf[0]) == -1.25 and float(buf[-1]) == 7.75 and (buf[1 + ec.VIEW_LEN:-1] == 0.5).all()
    assert np.array_equal(ec.bits(buf[1:1 + ec.VIEW_LEN]), ec.bits(ec.values(0)[0][ec.I_VIEW]))


def test_nan_and_inf_stay_in_their_elements(one_update):
    for i, s in enumerate(one_update["ema"].shadows):
        bad = np.flatnonzero(~np.isfinite(s.cpu().numpy()))
        assert bad.tolist() == (sorted((ec.NAN_AT, ec.PINF_AT, ec.NINF_AT)) if i == ec.I_NONFINITE else []), i
    s = one_update["ema"].shadows[ec.I_NONFINITE].cpu().numpy()
    assert np.isnan(s[ec.NAN_AT]) and s[ec.PINF_AT] == np.inf and np.isnan(s[ec.NINF_AT])          # (-Inf + Inf)


def test_two_runs_from_the_same_start_are_bitwise_equal(one_update):
    again, _, _ = _run_once()
    assert all(np.array_equal(ec.bits(a), ec.bits(b)) for a, b in zip(again.shadows, one_update["ema"].shadows))


def test_three_updates_with_warmup_use_the_weight_of_each_step():
    ema, params, _ = ec.make_ema("cuda", seed=1, decay=DECAY, warmup=True)
    ps, es = ec.values(1)
    want = [e.numpy() for e in es]
    weights = [weight_at(t, DECAY, True) for t in range(3)]
    assert weights == [float(np.float32(1.0 - d)) for d in (0.1, 2.0 / 11.0, 0.25)]
    for t in range(3):
        assert ema.num_updates == t and ema.decay_at() == [0.1, 2.0 / 11.0, 0.25][t]
        ema.update()
        want = ec.reference_update([torch.from_numpy(w) for w in want], ps, weights[t])
        ec.assert_same(ema.shadows, want, f"step {t}")
    assert ema.num_updates == 3


def test_swap_is_an_exact_exchange_and_twice_the_identity():
    ema, params, buf = ec.make_ema("cuda", decay=DECAY)
    ps, es = ec.values(0)
    versions = [p._version for p in params]
    edge = (ec.bits(buf[0]), ec.bits(buf[1 + ec.VIEW_LEN:]))
    ema.swap()
    assert ema.swapped is True
    assert all(np.array_equal(ec.bits(p), ec.bits(e)) for p, e in zip(params, es))
    assert all(np.array_equal(ec.bits(s), ec.bits(p)) for s, p in zip(ema.shadows, ps))
    assert int(ec.bits(ema.shadows[ec.I_NONFINITE])[ec.NAN_AT]) == ec.NAN_BITS                # the NaN's payload moved as it was
    assert all(p._version > v for p, v in zip(params, versions))
    assert np.array_equal(ec.bits(buf[0]), edge[0]) and np.array_equal(ec.bits(buf[1 + ec.VIEW_LEN:]), edge[1])
    assert all(np.array_equal(ec.bits(v), ec.bits(e)) for v, e in zip(ema.model_state_dict().values(), es))      # the averages, wherever they are
    with pytest.raises(RuntimeError, match="swapped in"):
        ema.update()
    assert ema.num_updates == 0
    versions = [p._version for p in params]
    ema.swap()
    assert ema.swapped is False
    assert all(np.array_equal(ec.bits(p), ec.bits(q)) for p, q in zip(params, ps))
    assert all(np.array_equal(ec.bits(s), ec.bits(e)) for s, e in zip(ema.shadows, es))
    assert int(ec.bits(params[ec.I_NONFINITE])[ec.NAN_AT]) == ec.NAN_BITS
    assert all(p._version > v for p, v in zip(params, versions))
    assert np.array_equal(ec.bits(buf[0]), edge[0]) and np.array_equal(ec.bits(buf[1 + ec.VIEW_LEN:]), edge[1])
    with pytest.raises(RuntimeError, match="boom"):
        with ema.averaged():
            assert ema.swapped
            raise RuntimeError("boom")
    assert ema.swapped is False and all(np.array_equal(ec.bits(p), ec.bits(q)) for p, q in zip(params, ps))      # swapped back in the finally


NET = dict(sigma_chn=1, n_feat=[32, 64], dep_S=3, n_resblocks=1)


def _net(seed):
    net = VIRAttResUNet(3, **NET)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=seed), strict=True)
    return net.cuda().eval()


def test_a_replaying_network_runs_on_the_averaged_weights_and_back():
    net = _net(11)
    ema = WeightEMA(net, decay=DECAY)
    second = synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=12)
    assert ema.names == list(second)
    with torch.no_grad():
        for name, s in zip(ema.names, ema.shadows):
            s.copy_(second[name])
    x = synth_images(2, 3, 18, 22).cuda()
    with torch.no_grad():
        for _ in range(4):
            live = [t.clone() for t in net(x)]
        assert graph.auto_stats(net)["replays"] >= 1
        fresh = VIRAttResUNet(3, **NET)
        fresh.load_state_dict(ema.model_state_dict(), strict=True)
        averaged = [t.clone() for t in fresh.cuda().eval()(x)]
        assert not torch.equal(averaged[0], live[0])
        for _ in range(2):                                       # once more in each direction: stale packed weights or a stale graph show here
            with ema.averaged():
                for _ in range(3):
                    assert all(torch.equal(a, b) for a, b in zip(net(x), averaged))
            for _ in range(3):
                assert all(torch.equal(a, b) for a, b in zip(net(x), live))
    assert not ema.swapped and all(torch.equal(s, second[n].cuda()) for n, s in zip(ema.names, ema.shadows))


def test_update_after_a_torch_adam_step():
    ps, es = ec.values(2, False)
    params, _ = ec.make_params(ps, "cuda")
    ema = WeightEMA(list(zip(ec.NAMES, params)), decay=0.9)
    opt = torch.optim.Adam(params, lr=1e-2)
    g = torch.Generator().manual_seed(9)
    want = [p.numpy() for p in ps]
    for t in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g).cuda()
        opt.step()
        ema.update()
        want = ec.reference_update([torch.from_numpy(w) for w in want], params, weight_at(t, 0.9))
        ec.assert_same(ema.shadows, want, f"adam step {t}")
    assert ema.num_updates == 2 and not any(np.array_equal(ec.bits(s), ec.bits(p)) for s, p in zip(ema.shadows, ps) if p.numel() > 8)


def test_no_host_synchronisation_in_twenty_updates():
    ema, _, _ = ec.make_ema("cuda", nonfinite=False, decay=DECAY, warmup=True)
    ema.update()                                                 # the warm-up: the library is loaded
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(20):
            ema.update()
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert ema.num_updates == 21 and all(bool(torch.isfinite(s).all()) for s in ema.shadows)
