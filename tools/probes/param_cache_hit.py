#!/usr/bin/env python
"""Host time of the parameter-cache HIT path, no device: ConvParam.packed() and ops._sft_weights on seeded caches, N calls each.

    python tools/probes/param_cache_hit.py [TREE] [N]

TREE: the checkout whose `virnet_amd` is timed (default: this one) -- works on trees from before and after ParamCache, so the two can be
run alternately (profiles/param_cache_refactor.md).  Prints one JSON line: ns per call, best of 5 repeats and their spread."""
import json
import os
import sys
import time

tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..", ".."))
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
sys.path.insert(0, tree)
import torch                                                                        # noqa: E402
from virnet_amd import _native as nat, ops                                          # noqa: E402
from virnet_amd.networks.AttResUNet import AttLayer                                 # noqa: E402
from virnet_amd.networks.params import ConvParam                                    # noqa: E402

assert os.path.abspath(ops.__file__).startswith(tree)
ops._dev_check = lambda t, name: None                                               # (the seeding miss runs the builders on CPU tensors)
ops.pack_weight = lambda w, b, **kw: "packing"
conv, att = ConvParam(96, 96, 3), AttLayer(96, 4)
assert conv.packed() == "packing" and conv.packed() == "packing"
first = ops._sft_weights(att)
assert ops._sft_weights(att)[0] is first[0]                                         # seeded: the second call is a hit


def ns_per_call(fn, arg=None):
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        if arg is None:
            for _ in range(n):
                fn()
        else:
            for _ in range(n):
                fn(arg)
        runs.append((time.perf_counter() - t0) / n * 1e9)
    return {"best": round(min(runs), 1), "worst": round(max(runs), 1)}


with torch.no_grad(), ops.forward_scope():                                          # as the engine calls them: knobs parsed once per scope
    out = {"packed": ns_per_call(conv.packed), "sft_weights": ns_per_call(ops._sft_weights, att)}
print(json.dumps({"tree": "ParamCache" if hasattr(conv, "_cache") else "parent", "calls": n, "ns_per_call": out}))
