"""One rank of the two-rank fit runs of tests/test_fit_dist_gpu.py: ``python fit_dist_worker.py RANK WORLD PORT OUT_DIR``.  Both ranks share
cuda:0 over gloo (one device here; RCCL needs one per rank).  Runs every scenario of tests/fit_dist_cases.py through ``fit_denoising`` /
``fit_sisr`` with the process group initialised, then the SISR resume, and writes ``OUT_DIR/rank<r>.pt``."""
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
    from virnet_amd import datagen, elbo, fit
    from virnet_amd import dist as vdist
    assert vdist.init(timeout=120)[2] == world
    results = {}

    def record_first(store):
        """the step-0 batch as the loop builds it: the first result of the batch makers (the real-noise loop's sigma_gt is the first
        noise_estimate, on the rank's rows of the mixed pair)"""
        real = {k: getattr(datagen, k) for k in ("denoise_batch", "real_batch", "sisr_batch")}
        real_ne = elbo.noise_estimate

        def wrap(key):
            def call(*a, **k):
                out = real[key](*a, **k)
                store.setdefault(key, [None if t is None else t.detach().cpu() for t in out])
                return out
            return call

        def ne(im_noisy, im_gt, *a, **k):
            out = real_ne(im_noisy, im_gt, *a, **k)
            store.setdefault("noise_estimate", [im_noisy.detach().cpu(), im_gt.detach().cpu(), out.detach().cpu()])
            return out
        for key in real:
            setattr(datagen, key, wrap(key))
        elbo.noise_estimate = ne

        def undo():
            for key, fn in real.items():
                setattr(datagen, key, fn)
            elbo.noise_estimate = real_ne
        return undo

    routes = {"finish": 0, "reduce_grads": 0}                  # which route averaged a step: the fused backward's finish() or reduce_grads()

    def counted(key):
        inner = getattr(vdist.GradientReducer, key)

        def call(self, *a, **k):
            routes[key] += 1
            return inner(self, *a, **k)
        return call
    for key in routes:
        setattr(vdist.GradientReducer, key, counted(key))

    for name, (task, _, is_real) in fc.SCENARIOS.items():
        routes.update(finish=0, reduce_grads=0)
        net, pool, cfg = fc.make(name)
        if rank == 1:                                          # rank 0's parameters must win: the broadcast is part of the run
            with torch.no_grad():
                for p in net.parameters():
                    p.mul_(0.5)
        first, lines = {}, []
        undo = record_first(first)
        try:
            if task == "sisr":
                cfg["epochs"] = 2
                out = fit.fit_sisr(net, pool, cfg, save_dir=os.path.join(out_dir, "sisr"), log=lines.append)
            else:
                out = fit.fit_denoising(net, pool, cfg, real=is_real, log=lines.append)
        finally:
            undo()
        results[name] = dict(rows=torch.from_numpy(out["rows"]), params=fc.flat_params(net), world=out["world"], rank=out["rank"], first=first, lines=lines,
                             checkpoints=out["checkpoints"], leftover=hasattr(net, "_grad_reducer"), routes=dict(routes))
    # SISR: one epoch + resume + one epoch (every rank loads rank 0's file onto its own device)
    net, pool, cfg = fc.make("sisr")
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
    cfg["epochs"] = 2
    out = fit.fit_sisr(net, pool, cfg, resume=os.path.join(out_dir, "sisr", "models", "model_1.pth"), log=lambda s: None)
    results["sisr_resume"] = dict(rows=torch.from_numpy(out["rows"]), params=fc.flat_params(net), epoch_start=out["epoch_start"])
    # a batch the world does not divide
    try:
        fit.fit_denoising(*fc.make("syn_fused")[:2], dict(fc.DEN_CFG, batch_size=3), log=lambda s: None)
        results["indivisible"] = None
    except ValueError as e:
        results["indivisible"] = str(e)
    torch.save(results, os.path.join(out_dir, f"rank{rank}.pt"))
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
