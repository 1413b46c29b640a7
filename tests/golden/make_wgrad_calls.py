#!/usr/bin/env python
"""tests/golden/wgrad_calls.json: what ops.conv_wgrad / ops.convt_wgrad ask of the library, RECORDED FROM THE COMMIT BEFORE
ops.wgrad_route_rule EXISTED (the table's "recorded_from" names it).

The table is not produced by the code it tests.  Procedure (CPU only, no device):

    git worktree add PARENT <the commit before wgrad_route_rule>           (or any copy of that commit's tree)
    make -C PARENT/virnet_amd/csrc                                         (or VIRNET_HIP_LIB=<a library built from the same csrc>)
    python tests/golden/make_wgrad_calls.py PARENT "<hash and subject of that commit>" > tests/golden/wgrad_calls.json

The recorder imports the PARENT's `virnet_amd` (never this tree's) and calls its weight gradients once per case on tiny CPU tensors
(torch.empty: only shapes matter).  What touches a device is stubbed (`Driver`): `_dev_check` accepts CPU tensors, `nat.stream_handle`
returns 0, `_workspace` hands out a CPU byte tensor, `_zeros` a CPU vector, `_timer_start` / `_timer_stop` keep (key, flops) without
events, and every launching entry point (LAUNCHERS) is a logger that returns 0.  The `*_bytes` sizers are host functions of the built
library and run for real, so the recorded sizes are the library's.  tests/test_wgrad_dispatch.py drives this tree through the same Driver.

A case is (shape id, bias_channels, offer, environment index, index into "traces": equal traces are stored once).  A trace holds, each list in call order (empty fields are not stored):
    calls   every C call: [symbol, arguments]; integers and floats as given, every pointer as a label -- x | dy | in_mul | in_add | dw | db |
            ctr (the fp32 kernel's counters) | s2d (the space-to-depth gradient) | ws:<tag> | T:xt | T:yt | T:yt.col | null -- mapped from
            data_ptr, never an address; a descriptor passed by reference is spelled out field by field
    ws      every workspace request [tag, bytes]
    zeros   every _zeros request (the order decides which slice of a zero_arena a bias gradient gets)
    zeroed  whether dw (and the counters) came from torch.zeros: the fp32 kernel accumulates
    timer   [key, flops] as bench.py reads them
    ret     the returned tensors as labels (T:yt.db: the emitted image's own sums) -- its length is the return arity
    images  the final [buf, db, col] of each offered TImage, as labels
    exc     [type, message] where the call raised
main() refuses to write a table in which a route (ROUTES) or a bias source (BIAS_SOURCES) never occurs, or which lacks the ValueError
for a T image of the wrong geometry, the same image silently dropped, or a few-channel layer taking the bf16 form of an emitted image.
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
import wgrad_cases as wc                                    # noqa: E402  (pure data)

KNOBS = ("VIRNET_CONV_FORM", "VIRNET_WGRAD_FORM", "VIRNET_WINOGRAD")
ENVS = [{}] + [{"VIRNET_CONV_FORM": f} for f in ("bf16", "f16x3", "wino", "direct")] + [{"VIRNET_WGRAD_FORM": "f32"}]
LAUNCHERS = ("virnet_chsplit", "virnet_chsplit_s2", "virnet_conv_wgrad_f16", "virnet_conv_wgrad_f16_db", "virnet_conv_wgrad_f16_s2",
             "virnet_conv_wgrad", "virnet_colsum", "virnet_colpart_reduce", "virnet_space_to_depth2")
OFFERS = ("none", "xt", "yt_db", "yt_col", "yt_nosums", "both", "otherform", "wronggeom", "released")
ROUTES = ("s1", "s2", "convt", "f32")
BIAS_SOURCES = ("chsplit_dy", "emitted_db", "emitted_partials", "bias_sums_s2", "phase_pass", "colsum")

# shape id -> (mode, ks, cin, cout, cx, cy, n, h, w, pre, bias_channels): wgrad_cases' rows, then one shape on the fp32 side of each condition
SHAPES = {r.id: (r.mode, 3 if r.mode != wc.CONVT else 2, r.cin, r.cout, r.cx, r.cy, r.n, r.h, r.w, r.pre, r.bias_channels) for r in wc.ROWS}
FALLBACK = {"fb-s1-h4": (wc.S1, 3, 32, 32, 32, 32, 2, 4, 16, 1, 32),          # four rows: no row ring
            "fb-s2-h4": (wc.S2, 3, 32, 64, 32, 64, 2, 4, 16, 1, 64),          # four LOW-resolution rows
            "fb-s2-cx40": (wc.S2, 3, 40, 32, 40, 32, 2, 6, 12, 2, 32),        # the phase image takes whole 32-channel blocks
            "fb-convt-c48": (wc.CONVT, 2, 64, 48, 64, 48, 2, 6, 12, 0, 48),   # ... of dy, for the transposed conv
            "fb-1x1": (wc.S1, 1, 32, 32, 32, 32, 2, 8, 8, 0, 32)}
SHAPES.update(FALLBACK)
# The cross product is thinned to what the routing can tell apart (every route, bias source and asymmetry still occurs: main() checks):
#   every shape, default environment, its bias_channels, no offer: the argument lists of all rows of wgrad_cases and the fallback shapes
CORE = ["kg2nwv1-s1-f16-c32to32-n2h5w32", "kg2nwv1-s2-f16-c32to32-n2h6w32", "kg2nwv1-convt-f16-c32to32-n2h7w32", "record-s1-f16-c96to3-n2h8w33"]
#   CORE (per mode the smallest instantiation row, and a 3-of-16 record row) and the fallback shapes: also without bias and in every environment;
#   CORE: every offer in the default environment; under bf16 every offer for the stride-1 rows (the record row is the few-channel layer an
#   emitted bf16 image widens), the image of the other operand form for the stride-2 rows


def cases():
    out = []
    for sid, shape in SHAPES.items():
        convt, bias = shape[0] == wc.CONVT, shape[10]
        out.append((sid, bias, "none", 0))
        if sid in CORE or sid in FALLBACK:
            out += [(sid, bias, "none", e) for e in range(1, len(ENVS))]
            if not convt:                                     # (convt_wgrad always returns the bias gradient)
                out += [(sid, None, "none", e) for e in (0, 1)]
        if sid in CORE:
            offers = [o for o in OFFERS[1:] if not convt or not o.startswith("yt") and o != "both"]      # (convt_wgrad takes xt only)
            out += [(sid, bias, o, e) for o in offers for e in (0, 1) if e == 0 or shape[0] == wc.S1 or o == "otherform"]
            if not convt:
                out += [(sid, None, o, 0) for o in ("yt_db", "yt_col", "yt_nosums")]
    out += [("fb-s1-h4", 32, "both", 0), ("fb-s2-h4", 64, "wronggeom", 0)]     # an offer on the fp32 route is not looked at
    return out


EMPTY = dict(calls=[], ws=[], zeros=[], zeroed={}, timer=[], ret=None, images={}, exc=None)


def slim(trace):
    """the trace as the table stores it: without its empty fields (test: dict(EMPTY, **stored))"""
    return {k: v for k, v in trace.items() if v != EMPTY[k]}


def route_of(trace):
    names = [c[0] for c in trace["calls"]]
    if "virnet_conv_wgrad_f16_s2" in names:
        mode = [c[1][11] for c in trace["calls"] if c[0] == "virnet_conv_wgrad_f16_s2"][0]
        return "convt" if mode else "s2"
    if "virnet_conv_wgrad_f16" in names or "virnet_conv_wgrad_f16_db" in names:
        return "s1"
    return "f32" if "virnet_conv_wgrad" in names else None


def contraction_bf16(trace):
    """the bf16 operand flag the f16-pipe contraction was launched with (None: fp32 route or no launch)"""
    at = {"virnet_conv_wgrad_f16": 11, "virnet_conv_wgrad_f16_db": 11, "virnet_conv_wgrad_f16_s2": 12}
    got = [bool(c[1][at[c[0]]]) for c in trace["calls"] if c[0] in at]
    return got[0] if got else None


def bias_source_of(trace):
    if trace["ret"] is None or len(trace["ret"]) < 2:
        return None
    names = [c[0] for c in trace["calls"]]
    if "virnet_conv_wgrad_f16_db" in names:
        return "emitted_partials"
    if "virnet_colpart_reduce" in names or (trace["ret"][1] == "T:yt.db" and route_of(trace) == "s2"):
        return "bias_sums_s2"
    if trace["ret"][1] == "T:yt.db":
        return "emitted_db"
    if "virnet_colsum" in names:
        return "colsum"
    if any(c[0] == "virnet_chsplit_s2" and c[1][13] > 0 for c in trace["calls"]):
        return "phase_pass"
    if any(c[0] == "virnet_chsplit" and c[1][0] == "dy" and c[1][13] > 0 for c in trace["calls"]):
        return "chsplit_dy"
    return None


class Driver:
    """`with Driver(virnet_amd.ops) as run:` -- run(case) = the trace of the tree's conv_wgrad / convt_wgrad for the case, without a device."""

    def __init__(self, ops):
        import torch
        self.torch, self.ops, self.nat = torch, ops, sys.modules[ops.__name__.rsplit(".", 1)[0] + "._native"]

    def __enter__(self):
        nat, ops, lib, torch, drv = self.nat, self.ops, self.nat.load(), self.torch, self
        argtypes = {name: types for name, _, types in nat.SYMBOLS}

        def spell(a, ctype):
            if isinstance(a, type(C.byref(C.c_int()))):        # a descriptor by reference: its fields, pointers as labels
                d = a._obj
                return [drv.label(getattr(d, f)) if t is C.c_void_p else getattr(d, f) for f, t in d._fields_]
            return drv.label(a) if ctype is C.c_void_p else a

        class Lib:                                             # the library with its launching entry points replaced by loggers
            def __getattr__(_, name):
                if name not in LAUNCHERS:
                    return getattr(lib, name)
                return lambda *args: drv.log["calls"].append([name, [spell(a, t) for a, t in zip(args, argtypes[name], strict=True)]]) or 0

        class Torch:                                           # ops' `torch` with the two allocators watched
            def __getattr__(_, name):
                return getattr(torch, name)

            def zeros(_, *a, **k):
                return drv.allocated(torch.zeros(*a, **k), True)

            def empty(_, *a, **k):
                return drv.allocated(torch.empty(*a, **k), False)

        def workspace(tag, nbytes, device):
            drv.log["ws"].append([tag, int(nbytes)])
            return drv.name(torch.empty(max(int(nbytes), 1), dtype=torch.uint8), "ws:" + tag)

        def zeros(n, device):
            drv.log["zeros"].append(int(n))
            return drv.name(torch.zeros(n, dtype=torch.float32), "db")

        self._saved = (nat._lib, nat.stream_handle, ops._dev_check, ops._workspace, ops._zeros, ops._timer_start, ops._timer_stop, ops._TIMER, ops.torch,
                       {k: os.environ.get(k) for k in KNOBS})
        nat._lib, nat.stream_handle, ops._dev_check, ops._workspace, ops._zeros = Lib(), (lambda: 0), (lambda t, name: None), workspace, zeros
        ops._timer_start, ops._timer_stop = (lambda: ()), (lambda ev, key, flops: drv.log["timer"].append([list(key), flops]))
        ops._TIMER, ops.torch = ops.LaunchTimer(), Torch()     # (a timer is set: the single-launch route records under one only)
        return self.run

    def __exit__(self, *exc):
        nat, ops = self.nat, self.ops
        (nat._lib, nat.stream_handle, ops._dev_check, ops._workspace, ops._zeros, ops._timer_start, ops._timer_stop, ops._TIMER, ops.torch, env) = self._saved
        self._environ(env)
        return False

    @staticmethod
    def _environ(env):
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in env.items() if v is not None})

    # ---- labels: every tensor of a case is kept alive until the case ends, so no address is handed out twice
    def name(self, t, label):
        self.keep.append(t)
        self.labels[t.data_ptr()] = label
        return t

    def label(self, p):
        p = getattr(p, "value", p)
        return "null" if not p else self.labels[p]

    def allocated(self, t, zeroed):
        what = "dw" if tuple(t.shape) == self.weight_shape else "ctr" if t.dtype == self.torch.int32 else "s2d"
        if what != "s2d":
            self.log["zeroed"][what] = zeroed
        return self.name(t, what)

    def run(self, case):
        torch, ops = self.torch, self.ops
        sid, bias, offer, env = case
        mode, ks, cin, cout, cx, cy, n, h, w, pre, _ = SHAPES[sid]
        self._environ(ENVS[env])
        self.log = log = json.loads(json.dumps(EMPTY))
        self.labels, self.keep = {}, []
        self.weight_shape = (cin, cout, 2, 2) if mode == wc.CONVT else (cout, cin, ks, ks)
        gx, gy = {wc.S1: ((n, h, w, cx), (n, h, w, cy)), wc.S2: ((n, 2 * h, 2 * w, cx), (n, h, w, cy)), wc.CONVT: ((n, h, w, cx), (n, 2 * h, 2 * w, cy))}[mode]
        x, dy = self.name(torch.empty(gx), "x"), self.name(torch.empty(gy), "dy")
        kw = dict(in_slope=0.2) if pre >= 1 else {}
        if pre == 2:
            kw.update(in_mul=self.name(torch.empty(n, cx), "in_mul"), in_add=self.name(torch.empty(n, cx), "in_add"))
        # the offered images: of the operand form the call would use (bf16 form, whole 32-channel blocks) unless the offer says otherwise
        bf = (ENVS[env].get("VIRNET_CONV_FORM") == "bf16" and min(cin, cout) >= 32) != (offer == "otherform")
        nsum = cout if bias is None else bias

        def image(which, geom, sums):
            gn, gh, gw, gc = geom
            t = ops.TImage(None if offer == "released" else self.name(torch.empty(16, dtype=torch.uint8), "T:" + which),
                           gn, gh + (offer == "wronggeom"), gw, gc, bf)
            if sums == "db":
                t.db = self.name(torch.zeros(nsum), "T:%s.db" % which)
            elif sums == "col":
                t.col, t.nblk, t.ncol = self.name(torch.empty(64), "T:%s.col" % which), 7, nsum
            return t

        imgs = {}
        if offer in ("xt", "both", "otherform", "wronggeom", "released"):
            imgs["xt"] = image("xt", gx, None)
        if mode != wc.CONVT and offer != "xt" and offer != "none":
            imgs["yt"] = image("yt", gy, "col" if offer == "yt_col" else None if offer == "yt_nosums" else "db")
        try:
            if mode == wc.CONVT:
                ret = ops.convt_wgrad(x, dy, self.weight_shape, **imgs)
            else:
                ret = ops.conv_wgrad(x, dy, self.weight_shape, stride=2 if mode == wc.S2 else 1, bias_channels=bias, **kw, **imgs)
            log["ret"] = [self.label(t.data_ptr()) for t in (ret if isinstance(ret, tuple) else (ret,))]
        except Exception as e:                                 # noqa: BLE001  (whatever it raises is the behaviour recorded)
            log["exc"], log["zeroed"] = [type(e).__name__, str(e)], {}      # (no dw comes back: how one was allocated on the way says nothing)
        log["images"] = {k: [None if v is None else self.label(v.data_ptr()) for v in (t.buf, t.db, t.col)] for k, t in imgs.items()}
        self.keep = []
        return log


def main():
    tree, commit = os.path.abspath(sys.argv[1]), sys.argv[2]
    sys.path.insert(0, tree)
    from virnet_amd import ops
    assert os.path.abspath(ops.__file__).startswith(tree), "virnet_amd was imported from somewhere else"
    assert not hasattr(ops, "wgrad_route_rule"), "this tree already has the rule the table is to test: give the commit before it"
    with Driver(ops) as run:
        table = [list(c) + [run(c)] for c in cases()]
    traces = [r[4] for r in table]
    for route in ROUTES:
        assert any(route_of(t) == route for t in traces), f"route {route} never taken"
    for src in BIAS_SOURCES:
        assert any(bias_source_of(t) == src for t in traces), f"bias source {src} never used"
    wrong = [t for r, t in zip(table, traces) if r[2] == "wronggeom"]
    assert any(t["exc"] and t["exc"][0] == "ValueError" for t in wrong), "no ValueError for a T image of the wrong geometry"
    assert any(t["exc"] is None and route_of(t) in ("s2", "convt") and any(c[0] == "virnet_chsplit" for c in t["calls"]) for t in wrong), \
        "no case in which a T image of the wrong geometry is silently dropped"
    assert any(route_of(t) == "s1" and contraction_bf16(t) and min(SHAPES[r[0]][2:4]) < 32 for r, t in zip(table, traces)), \
        "no few-channel stride-1 layer widened to bf16 by an emitted bf16 image"
    stored = []
    for r, t in zip(table, traces):
        t = slim(t)
        if t not in stored:
            stored.append(t)
        r[4] = stored.index(t)
    rows = lambda items: ",\n".join("  " + json.dumps(i, separators=(",", ":")) for i in items)     # noqa: E731
    sys.stdout.write("{\n \"recorded_from\": %s,\n \"envs\": %s,\n \"columns\": [\"shape\", \"bias_channels\", \"offer\", \"env\", \"trace\"],\n"
                     " \"cases\": [\n%s\n ],\n \"traces\": [\n%s\n ]\n}\n" % (json.dumps(commit), json.dumps(ENVS), rows(table), rows(stored)))
    print("%d cases" % len(table), file=sys.stderr)


if __name__ == "__main__":
    main()
