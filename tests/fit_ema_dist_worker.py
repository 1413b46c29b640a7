"""One rank of the two-rank weight-average run of tests/test_fit_ema_gpu.py: ``python fit_ema_dist_worker.py RANK WORLD PORT OUT_DIR``.  Both
ranks share cuda:0 over gloo, as in tests/fit_dist_worker.py.  Runs the ``syn_fused`` scenario of tests/fit_dist_cases.py through
``fit_denoising`` with ``ema_decay``, then once more with one shadow of rank 1 perturbed after the second update, and writes
``OUT_DIR/rank<r>.pt``."""
import os
import sys


def main():
    rank, world, port, out_dir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      VIRNET_DIST_BACKEND="gloo")
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import torch
    import fit_dist_cases as fc
    from virnet_amd import dist as vdist
    from virnet_amd import ema as vema
    from virnet_amd import fit
    assert vdist.init(timeout=120)[2] == world
    results = {}

    net, pool, cfg = fc.make("syn_fused")
    if rank == 1:                                              # rank 0's parameters must win: the shadows are cloned after the broadcast
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(0.5)
    lines = []
    out = fit.fit_denoising(net, pool, dict(cfg, ema_decay=0.9), save_dir=os.path.join(out_dir, "ema"), log=lines.append)
    avg = out["ema"]
    results["run"] = dict(params=fc.flat_params(net), shadows=torch.cat([s.reshape(-1) for s in avg.shadows]).cpu(), num_updates=avg.num_updates,
                          swapped=avg.swapped, checkpoints=out["checkpoints"], lines=lines, world=out["world"], rank=out["rank"])

    # the same run with one element of one shadow moved on rank 1 after the second update: the epoch's comparison must refuse it on every rank
    update, calls = vema.WeightEMA.update, [0]

    def perturbed(self):
        update(self)
        calls[0] += 1
        if rank == 1 and calls[0] == 2:
            with torch.no_grad():
                self.shadows[3].view(-1)[0] += 1.0
    vema.WeightEMA.update = perturbed
    net, pool, cfg = fc.make("syn_fused")
    try:
        fit.fit_denoising(net, pool, dict(cfg, ema_decay=0.9), log=lambda s: None)
        results["perturbed"] = None
    except RuntimeError as e:
        results["perturbed"] = str(e)
    finally:
        vema.WeightEMA.update = update
    results["updates_before_the_refusal"] = calls[0]
    results["leftover"] = hasattr(net, "_grad_reducer")
    torch.save(results, os.path.join(out_dir, f"rank{rank}.pt"))
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
