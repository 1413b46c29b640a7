#!/usr/bin/env python
"""tests/golden/pack_images.json: which images ops.pack_weight packs, RECORDED FROM THE COMMIT BEFORE ops.pack_images_rule EXISTED.

The table is not produced by the function it tests.  Procedure (CPU only, no device):

    git worktree add PARENT <the commit before pack_images_rule>          (or any copy of that commit's tree)
    make -C PARENT/virnet_amd/csrc                                         (or VIRNET_HIP_LIB=<a library built from the same csrc>)
    python tests/golden/make_pack_images.py PARENT > tests/golden/pack_images.json

The recorder imports the PARENT's `virnet_amd` (never this tree's) and calls its `ops.pack_weight` once per row and environment with a
weight on the `meta` device (shapes only).  What the parent would have touched a device for is stubbed (`Driver`): `_dev_check` accepts
everything, `nat.ptr` / `nat.stream_handle` return 0 and the library's `virnet_pack_*` entry points -- the only ones that write device
memory -- return 0 without doing anything.  `virnet_conv_get_plan` and the `*_weight_floats` sizers are host functions of the built
library and run for real, so the recorded sizes and plan fields are the library's.  tests/test_pack_images.py drives this tree's
pack_weight through the same `Driver`.

A row is (kind, stride, ks, cin, cout) of the FORWARD layer; kind is conv | convt | conv_dgrad | convt_dgrad.  The grid is small and kept
whole: rows() x ENVS.  Per row and environment the table holds the packing as `packing()` spells it: the base image's numel, the scalar
fields (ks, cout, cin_real, cin_pad, n_pad, nrep, transposed), {image: numel} of the images present, and the same of the nested `s2`
packing.  main() refuses to write a table in which an image a kind can carry (CARRIES) is never present or never absent.
"""
import json
import os
import sys

ENTRY = [(3, 64), (4, 96), (7, 96), (8, 96), (9, 96), (8, 128), (16, 96)]      # both sides of cin <= 8 and cout <= 96
CC = [(c, c) for c in (32, 64, 96, 160, 192, 224, 288)]
EXIT = [(64, 1), (96, 3), (96, 4), (96, 16), (96, 32), (96, 48)]               # both sides of cout*9 <= 32, cout <= 32 and cout % 32
FORWARD = ([("conv", 1, 3, ci, co) for ci, co in ENTRY + CC + EXIT] + [("conv", 1, 1, 4, 8), ("conv", 1, 1, 16, 64)] +
           [("conv", 2, 3, ci, co) for ci, co in ((64, 128), (96, 192), (96, 48), (24, 64))] +
           [("convt", 2, 2, ci, co) for ci, co in ((192, 96), (128, 64), (96, 48), (24, 32))])
ENVS = [{}] + [{"VIRNET_CONV_FORM": f} for f in ("wx4", "f16x3", "wino", "direct", "bf16")] + [{"VIRNET_WINOGRAD": "0"}, {"VIRNET_WINOGRAD": "1"}]
KNOBS = ("VIRNET_CONV_FORM", "VIRNET_WINOGRAD")
IMAGES = ("wino", "f16", "bf16", "wx4", "exit", "entry")                       # the tensor images of a PackedWeight; `s2` is a packing
CARRIES = {"conv": IMAGES, "convt": ("f16",), "conv_dgrad": ("wino", "f16", "bf16", "wx4"), "convt_dgrad": ("s2",)}
COLUMNS = ("kind", "stride", "ks", "cin", "cout", "one packing per environment")
FIELDS = ("ks", "cout", "cin_real", "cin_pad", "n_pad", "nrep", "transposed")


def packing(pw) -> dict:
    out = {"w": pw.w.numel(), "fields": [int(getattr(pw, f)) for f in FIELDS],
           "images": {k: getattr(pw, k).numel() for k in IMAGES if getattr(pw, k) is not None}}
    if pw.s2 is not None:
        out["s2"] = packing(pw.s2)
    return out


class Driver:
    """`with Driver(virnet_amd.ops) as run:` -- run(row, env) = packing() of the tree's pack_weight for the row, without a device."""

    def __init__(self, ops):
        import torch
        self.torch, self.ops, self.nat = torch, ops, sys.modules[ops.__name__.rsplit(".", 1)[0] + "._native"]

    def __enter__(self):
        nat, ops, lib = self.nat, self.ops, self.nat.load()

        class Lib:                                             # the library with its device-touching pack entry points cut out
            def __getattr__(_, name):
                return (lambda *args: 0) if name.startswith("virnet_pack_") else getattr(lib, name)

        self._saved = (nat._lib, nat.ptr, nat.stream_handle, ops._dev_check, {k: os.environ.get(k) for k in KNOBS})
        nat._lib, nat.ptr, nat.stream_handle, ops._dev_check = Lib(), (lambda t: 0), (lambda: 0), (lambda t, name: None)
        return self.run

    def __exit__(self, *exc):
        nat, ops = self.nat, self.ops
        nat._lib, nat.ptr, nat.stream_handle, ops._dev_check, env = self._saved
        self._environ(env)
        return False

    @staticmethod
    def _environ(env):
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in env.items() if v is not None})

    def run(self, row, env):
        kind, stride, ks, cin, cout = row
        self._environ(env)
        shape = (cin, cout, ks, ks) if kind.startswith("convt") else (cout, cin, ks, ks)
        w = self.torch.empty(shape, dtype=self.torch.float32, device="meta")
        if kind.endswith("_dgrad"):                            # as ConvParam.packed_dgrad calls it
            return packing(self.ops.pack_weight(w, None, transposed=kind == "convt_dgrad", dgrad=True))
        b = self.torch.empty(cout, dtype=self.torch.float32, device="meta")
        return packing(self.ops.pack_weight(w, b, transposed=kind == "convt", stride=stride))


def rows(run):
    """FORWARD plus the input gradient of every row of it that pack_weight(dgrad=True) accepts"""
    out = list(FORWARD)
    for kind, stride, ks, cin, cout in FORWARD:
        row = (kind + "_dgrad", stride, ks, cin, cout)
        try:
            run(row, {})
        except ValueError:
            continue
        out.append(row)
    return out


def main():
    tree = os.path.abspath(sys.argv[1])
    sys.path.insert(0, tree)
    from virnet_amd import ops
    assert os.path.abspath(ops.__file__).startswith(tree), "virnet_amd was imported from somewhere else"
    assert not hasattr(ops, "pack_images_rule"), "this tree already has the function the table is to test: give the commit before it"
    with Driver(ops) as run:
        table = [list(row) + [[run(row, env) for env in ENVS]] for row in rows(run)]
    for kind, names in CARRIES.items():
        got = [set(p["images"]) | ({"s2"} if "s2" in p else set()) for r in table if r[0] == kind for p in r[5]]
        assert got, kind
        for name in names:
            assert any(name in g for g in got) and any(name not in g for g in got), f"{kind}: {name} is always or never there"
        assert set().union(*got) <= set(names), (kind, set().union(*got))
    sys.stdout.write("{\n \"fields\": %s,\n \"envs\": %s,\n \"columns\": %s,\n \"rows\": [\n" % (json.dumps(FIELDS), json.dumps(ENVS), json.dumps(COLUMNS)) +
                     ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in table) + "\n ]\n}\n")
    print("%d rows x %d environments" % (len(table), len(ENVS)), file=sys.stderr)


if __name__ == "__main__":
    main()
