#!/usr/bin/env python
"""Host cost of the weight-gradient dispatch alone, on the CPU: the default-environment cases of tests/golden/wgrad_calls.json without an
offered image (what a training step calls) through the recorder's Driver (launches replaced by loggers, so its own cost is in every
figure), ten passes per repeat: microseconds per call inside ops.conv_wgrad / ops.convt_wgrad.
    python tools/probes/wgrad_host_time.py [TREE] [repeats]"""
import importlib.util
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, os.pardir)
tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else ROOT)
sys.path.insert(0, tree)
from virnet_amd import ops  # noqa: E402

assert os.path.abspath(ops.__file__).startswith(tree), ops.__file__
spec = importlib.util.spec_from_file_location("make_wgrad_calls", os.path.join(ROOT, "tests", "golden", "make_wgrad_calls.py"))
rec = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rec)
cases = [c for c in rec.cases() if c[2] == "none" and c[3] == 0] * 10
spent = [0.0]


def timed(fn):
    def call(*a, **k):
        t0 = time.perf_counter()
        try:
            return fn(*a, **k)
        finally:
            spent[0] += time.perf_counter() - t0
    return call


conv_wgrad = ops.conv_wgrad                                  # (convt_wgrad's fallback calls it: counted once, in the outer call)
ops.convt_wgrad = timed(ops.convt_wgrad)
with rec.Driver(ops) as run:
    for c in cases:
        run(c)
    for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 5):
        spent[0] = 0.0
        for c in cases:
            ops.conv_wgrad = timed(conv_wgrad) if rec.SHAPES[c[0]][0] != rec.wc.CONVT else conv_wgrad
            run(c)
        dt = spent[0]
        print("%s: %d calls %.1f us/call" % (os.path.basename(tree), len(cases), 1e6 * dt / len(cases)))
