#!/usr/bin/env python
"""tests/golden/conv_forms.json: which kernel family ops.conv_mfma launches, RECORDED FROM THE COMMIT BEFORE ops.conv_form_rule EXISTED.

The table is not produced by the function it tests.  Procedure (CPU only, no device):

    git worktree add PARENT <the commit before conv_form_rule>            (or any copy of that commit's tree)
    make -C PARENT/virnet_amd/csrc                                         (or VIRNET_HIP_LIB=<a library built from the same csrc>)
    python tests/golden/make_conv_forms.py PARENT > tests/golden/conv_forms.json

The recorder imports the PARENT's `virnet_amd` (never this tree's) and calls its `ops.conv_mfma` once per row with tensors on the `meta`
device (shapes only) and a hand-built PackedWeight that carries the row's images.  What the parent would have touched a device for is
stubbed: `_dev_check` (accepts everything), `nat.ptr` (1 for a tensor, 0 for None), the T-buffer and workspace allocators `t_acquire` /
`_workspace` (meta tensors) and `_launch_conv`, which records the `form` it is handed instead of launching.  `virnet_conv_emit_ok` is a
host function of the built library and runs for real; the recorder wraps it only to note the tile form it is asked about (2 -> 8 rows,
1 -> 16 rows), which is the emitting tile height the parent computed.  A launch that never asks (no emission wanted, VIRNET_T_EMIT=0, a
form other than wx4) records 0 rows.

The grid is the product of LAYERS x their image sets x BATCHES x SIDES x operand combinations (res, mask, mul/add, in_mul/in_add, in_slope,
the three legal want_raw / want_act pairs) x EMITS x KNOBS: 7.5 million launches.  A line of the table is one launch spec -- everything
but the last two factors -- with the parent's answer under every emission kind x knob setting (78 rows of the product per line).  It holds
a fixed 1-in-SAMPLE sample of the 96 768 specs (crc32 of the spec, so it does not depend on iteration order) plus the specs of `curated()`,
the layers and launch sizes where the rule has the most branches.  `branches()` names the branch of the rule each row went
through -- from the row's inputs and what the parent did with and without the emission -- and main() refuses to write a table that misses
one.  The whole product, not only the sample, went once through the parent's conv_mfma and once through ops.conv_form_rule
(`make_conv_forms.py <tree> --all [part parts]` prints a digest of either): the same digest.
"""
import itertools
import json
import os
import sys
import zlib

# name -> (transposed, stride, input channels c (= cin_pad), pw.cout, stored channels, ks, the image sets the layer is tried with)
CC_IMAGES = ("", "wino", "f16", "f16+bf16", "f16+wx4", "wx4", "wino+f16+bf16+wx4")
LAYERS = {("cc%d" % c): (0, 1, c, c, c, 3, CC_IMAGES) for c in (64, 96, 160, 192, 224, 288)}
LAYERS.update({
    "entry": (0, 1, 16, 96, 96, 3, ("", "f16", "f16+wx4")),             # a 16-channel record -> features
    "exit": (0, 1, 96, 3, 3, 3, ("", "f16")),                           # a few-channel layer through conv_mfma (cout not whole blocks)
    "thin_dgrad": (0, 1, 96, 4, 32, 3, ("", "f16")),                    # input gradient of a few-channel layer: out_channels=32
    "s2": (0, 2, 96, 192, 192, 3, ("", "f16")),                         # DownBlock.downsampler
    "convt": (1, 1, 192, 96, 96, 1, ("", "f16")),                       # UpBlock.upsampler
    "convt_dgrad": (0, 2, 96, 192, 192, 3, ("", "f16", "f16+wx4")),     # its input gradient through pw.s2: a 3x3 stride-2 conv of dy
})
BATCHES = (1, 4, 32)
SIDES = ((16, 16), (17, 33), (48, 96), (64, 64), (128, 128), (256, 256))
OPERANDS = ("res", "mask", "mul", "in_mul", "in_slope")
WANTS = ("raw", "act", "both")
EMITS = (0, 1, 2)                                                        # none | plain | act + colsum
KNOBS = [{}] + [{"VIRNET_CONV_FORM": f} for f in ("wx4", "f16x3", "wino", "direct", "bf16")] + [
    {"VIRNET_WINOGRAD": "0"}, {"VIRNET_WINOGRAD": "1"}, {"VIRNET_DETERMINISTIC": "1"}, {"VIRNET_CONV_FORM": "f16x3", "VIRNET_DETERMINISTIC": "1"},
    {"VIRNET_WX4_MIN_WGS": "0"}, {"VIRNET_WX4_MIN_WGS": "64"}, {"VIRNET_WX4_MIN_WGS": "100000"}, {"VIRNET_WX4_MIN_WGS": "64", "VIRNET_WX4_EMIT_ROWS": "16"},
    {"VIRNET_WX4_MIN_COUT": "32"}, {"VIRNET_WX4_MIN_COUT": "128"}, {"VIRNET_WX4_MIN_FILL": "0.9"}, {"VIRNET_WX4_MIN_FILL": "0"},
    {"VIRNET_WX4_MIN_TILES": "8"}, {"VIRNET_WX4_MIN_SLAB_WGS": "0"}, {"VIRNET_WX4_MIN_SLAB_WGS": "100000"}, {"VIRNET_WX4_ROWS": "16"},
    {"VIRNET_WX4_ROWS": "8"}, {"VIRNET_WX4_EMIT_ROWS": "16"}, {"VIRNET_T_EMIT": "0"}, {"VIRNET_T_EMIT": "0", "VIRNET_WX4_MIN_WGS": "0"}]
ALL_KNOBS = sorted({k for kn in KNOBS for k in kn})
SAMPLE = 1200
CODES = {"direct": "d", "wino": "w", "f16x3": "f", "bf16": "b", "wx4": "x"}      # a result is written as code + emit rows: "x8", "f0"
FIELDS = ["layer", "images", "n", "h", "w", "operands", "want", "results: one per (emit, knobs) in itertools.product(emits, knobs), as code + emit rows"]


def specs():
    for layer, spec in LAYERS.items():
        for images, n, (h, w) in itertools.product(spec[6], BATCHES, SIDES):
            for bits in range(1 << len(OPERANDS)):
                operands = "+".join(o for i, o in enumerate(OPERANDS) if bits >> i & 1)
                for want in WANTS:
                    yield [layer, images, n, h, w, operands, want]


def rows_of(spec):
    return [spec + [emit, knobs] for emit, knobs in itertools.product(EMITS, KNOBS)]


def product():
    for spec in specs():
        yield from rows_of(spec)


def sampled(spec) -> bool:
    return zlib.crc32(json.dumps(spec).encode()) % SAMPLE == 0


def curated():
    """the C->C layers with the split-fp16 and Winograd images at launch sizes on both sides of the thresholds -- (4, 64, 64) x 160 channels
    is the 64-workgroup launch that VIRNET_WX4_MIN_WGS=64 admits to the Winograd form and the emission's own bound of 128 sends back."""
    shapes = ((4, 64, 64), (1, 128, 128), (1, 256, 256), (32, 128, 128), (6, 64, 64), (32, 17, 33))
    for n, h, w in shapes:
        for operands, want in (("", "raw"), ("in_slope", "act"), ("in_mul+in_slope", "act"), ("res", "raw"), ("mul", "both"), ("mul", "act"), ("mask", "raw")):
            yield ["cc96", "f16+wx4", n, h, w, operands, want]
    for layer, images in (("cc64", "f16+wx4"), ("cc192", "f16+wx4"), ("cc160", "f16+wx4"), ("cc96", "wx4"), ("entry", "f16+wx4")):
        for (n, h, w), operands, want in ((shapes[0], "", "raw"), (shapes[1], "in_slope", "act"), (shapes[2], "in_slope", "act")):
            yield [layer, images, n, h, w, operands, want]
    # the layers of a U-Net level that are not stride-1 C->C: up- and down-sampler, their input gradients, the few-channel ends
    yield from (["convt", "f16", 1, 64, 64, "res", "raw"], ["convt", "f16", 4, 64, 64, "", "act"], ["convt", "f16", 1, 64, 64, "res", "both"],
                ["s2", "f16", 1, 128, 128, "in_slope", "raw"], ["s2", "f16", 4, 128, 128, "res+in_slope", "raw"], ["convt_dgrad", "f16", 4, 128, 128, "", "raw"],
                ["thin_dgrad", "f16", 4, 128, 128, "", "raw"], ["exit", "f16", 1, 64, 64, "", "raw"], ["entry", "f16", 4, 128, 128, "", "act"])


class Parent:
    """The parent commit's conv_mfma, driven without a device."""

    def __init__(self, tree: str):
        sys.path.insert(0, os.path.abspath(tree))
        import torch
        from virnet_amd import _native as nat, ops
        assert os.path.abspath(ops.__file__).startswith(os.path.abspath(tree)), "virnet_amd was imported from somewhere else"
        assert not hasattr(ops, "conv_form_rule"), "this tree already has the function the table is to test: give the commit before it"
        self.torch, self.nat, self.ops = torch, nat, ops
        self.seen = {}
        lib = nat.load()

        class Lib:                                            # the library, noting which tile form conv_mfma asks virnet_conv_emit_ok about
            def __getattr__(_, name):
                return getattr(lib, name)

            def virnet_conv_emit_ok(_, d, form, nblk):
                self.seen["asked"] = form
                return lib.virnet_conv_emit_ok(d, form, nblk)

        nat._lib = Lib()
        nat.ptr = lambda t: 0 if t is None else 1
        nat.stream_handle = lambda: 0
        ops._dev_check = lambda t, name: None
        ops._workspace = lambda tag, nbytes, device: torch.empty(nbytes, dtype=torch.uint8, device="meta")
        ops.t_acquire = lambda n, h, w, c, bf16, device: ops.TImage(torch.empty(1, dtype=torch.uint8, device="meta"), n, h, w, c, bf16, None, False)
        ops._launch_conv = self.launch

    def launch(self, d, flops, what, form="direct", te=None):
        self.seen["form"], self.seen["te"] = form, te

    def run(self, row, emit=None):
        """(form, emit rows) of the row, with its own emission kind or the one given"""
        layer, images, n, h, w, operands, want, emit_row, knobs = row
        emit = emit_row if emit is None else emit
        transposed, stride, c, cout, cstore, ks, _ = LAYERS[layer]
        torch, ops = self.torch, self.ops
        t = lambda *shape: torch.empty(shape, dtype=torch.float32, device="meta")
        img = {k: t(1) for k in images.split("+") if k}
        pw = ops.PackedWeight(t(1), t(cout), ks, cout, c, c, (4 if transposed else 1) * ((cout + 31) // 32 * 32), 1, bool(transposed), **img)
        oh, ow = (2 * h, 2 * w) if transposed else (h // stride, w // stride)
        have = operands.split("+")
        kw = dict(stride=stride, want_raw=want in ("raw", "both"), want_act=want in ("act", "both"))
        if "res" in have:
            kw["res"] = t(n, oh, ow, cstore)
        if "mask" in have:
            kw["mask"] = t(n, oh, ow, cstore)
        if "mul" in have:
            kw["mul"], kw["add"] = t(n, cstore), t(n, cstore)
        if "in_mul" in have:
            kw["in_mul"], kw["in_add"] = t(n, c), t(n, c)
        if "in_slope" in have or "in_mul" in have:
            kw["in_slope"] = 0.2
        if cstore != cout:
            kw["out_channels"] = cstore
        if emit:
            kw["emit"] = dict(act=0.2, colsum=cstore) if emit == 2 else dict()
        for k in ALL_KNOBS:
            os.environ.pop(k, None)
        os.environ.update(knobs)
        self.seen.clear()
        ops.conv_mfma(t(n, h, w, c), pw, **kw)
        form, te, asked = self.seen["form"], self.seen["te"], self.seen.get("asked", 0)
        rows = {0: 0, 1: 16, 2: 8}[asked]
        assert (asked == 0 or form == "wx4") and (te is None or te.rows == rows), (row, self.seen)
        return form, rows


def branches(row, form, rows, plain_form):
    """names of the rule's branches the row went through (`plain_form`: what the parent launches for the same row without an emission)"""
    layer, images, n, h, w, operands, want, emit, knobs = row
    transposed, stride, c, cout, cstore, _, _ = LAYERS[layer]
    out = []
    if transposed:
        out.append("transposed:" + plain_form)
    elif stride == 2:
        out.append("stride2:" + plain_form)
    elif cstore != cout:
        out.append("padded_store:" + plain_form)
    else:
        want_form = knobs.get("VIRNET_CONV_FORM") or {None: "wx4", "0": "direct"}.get(knobs.get("VIRNET_WINOGRAD"), "wino")
        out.append("stride1:want_%s:%s" % (want_form, plain_form))
        if want_form == "wx4" and "wx4" in images and plain_form != "wx4":
            out.append("wx4_shape_refused")
        if cout % 32 and "f16" in images and want_form in ("wx4", "f16x3", "bf16"):
            out.append("cout_not_whole_blocks:" + plain_form)
    if emit and plain_form == "wx4":
        wgs = n * ((h + 15) // 16) * ((w + 31) // 32) * ((cout + 95) // 96)
        pinned = knobs.get("VIRNET_DETERMINISTIC") == "1" or knobs.get("VIRNET_WX4_MIN_WGS") == "0"
        if form == "f16x3":
            out.append("emit_back_to_f16x3:" + ("in_mul" if "in_mul" in operands else "c<32" if c < 32 else "below_128_wgs"))
            if 64 <= wgs < 128 and knobs.get("VIRNET_WX4_MIN_WGS") == "64":
                out.append("emit_back_to_f16x3:the_literal_128_under_MIN_WGS=64")
        else:
            out.append("emit_stays_wx4:" + ("no_f16_image" if "f16" not in images.split("+") else "pinned" if wgs < 128 and pinned else "fills_the_chip"))
            why = ("T_EMIT=0" if knobs.get("VIRNET_T_EMIT") == "0" else "EMIT_ROWS=16" if knobs.get("VIRNET_WX4_EMIT_ROWS") == "16" else
                   "DETERMINISTIC" if knobs.get("VIRNET_DETERMINISTIC") == "1" else "MIN_WGS=0" if knobs.get("VIRNET_WX4_MIN_WGS") == "0" else
                   "ROWS=16" if knobs.get("VIRNET_WX4_ROWS") == "16" else "default")
            out.append("emit_rows_%d:%s" % (rows, why))
    elif emit:
        out.append("emit_asked_of:" + form)
    return out


EVERY_BRANCH = (["transposed:f16x3", "transposed:direct", "stride2:f16x3", "stride2:direct", "padded_store:direct", "wx4_shape_refused", "cout_not_whole_blocks:direct"] +
                ["stride1:want_%s:%s" % (a, b) for a, b in (("wx4", "wx4"), ("wx4", "f16x3"), ("wx4", "direct"), ("f16x3", "f16x3"), ("f16x3", "direct"),
                                                            ("wino", "wino"), ("wino", "direct"), ("direct", "direct"), ("bf16", "bf16"), ("bf16", "f16x3"),
                                                            ("bf16", "direct"))] +
                ["emit_back_to_f16x3:" + s for s in ("in_mul", "c<32", "below_128_wgs", "the_literal_128_under_MIN_WGS=64")] +
                ["emit_stays_wx4:" + s for s in ("no_f16_image", "pinned", "fills_the_chip")] +
                ["emit_rows_8:default", "emit_rows_0:T_EMIT=0"] + ["emit_rows_16:" + s for s in ("EMIT_ROWS=16", "DETERMINISTIC", "MIN_WGS=0", "ROWS=16")] +
                ["emit_asked_of:" + f for f in ("direct", "wino", "f16x3", "bf16")])


def digest(tree):
    """--all: sha256 over (form, emit rows) of the WHOLE product (or of part I of N of it), from the tree's conv_mfma when the tree is the
    parent, from its ops.conv_form_rule when it has one: the two digests are equal."""
    import hashlib
    if os.path.exists(os.path.join(tree, "tests", "test_conv_form.py")):
        sys.path[:0] = [os.path.abspath(tree), os.path.join(os.path.abspath(tree), "tests")]
        import test_conv_form
        run = lambda row: test_conv_form.rule_of(row, LAYERS[row[0]][:5], os.environ)
    else:
        run = Parent(tree).run
    part, parts = (int(v) for v in (sys.argv[3:5] or (0, 1)))
    sha, total = hashlib.sha256(), 0
    for i, row in enumerate(product()):
        if i % parts == part:
            sha.update(("%s %d\n" % tuple(run(row))).encode())
            total += 1
    print("part %d of %d: %d rows, sha256 %s" % (part, parts, total, sha.hexdigest()))


def main():
    if len(sys.argv) > 2 and sys.argv[2] == "--all":
        return digest(sys.argv[1])
    parent = Parent(sys.argv[1])
    lines, seen, hits, knobs_seen = [], set(), {}, set()
    for spec in itertools.chain(curated(), (sp for sp in specs() if sampled(sp))):
        if json.dumps(spec) in seen:
            continue
        seen.add(json.dumps(spec))
        results = []
        for row in rows_of(spec):
            form, emit_rows = parent.run(row)
            for b in branches(row, form, emit_rows, parent.run(row, emit=0)[0] if row[7] else form):
                hits[b] = hits.get(b, 0) + 1
            results.append(CODES[form] + str(emit_rows))
        lines.append(spec + [" ".join(results)])
    missing = [b for b in EVERY_BRANCH if b not in hits]
    assert not missing and not set(hits) - set(EVERY_BRANCH), (missing, set(hits) - set(EVERY_BRANCH))
    assert {sp[0] for sp in lines} == set(LAYERS)
    layers = {k: dict(zip(("transposed", "stride", "c", "cout", "cstore"), v[:5])) for k, v in LAYERS.items()}
    head = {"fields": FIELDS, "codes": CODES, "emits": list(EMITS), "knobs": KNOBS, "layers": layers, "branch_hits": dict(sorted(hits.items()))}
    sys.stdout.write("{\n" + "".join(" %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in head.items()) + " \"specs\": [\n" +
                     ",\n".join("  " + json.dumps(sp, separators=(",", ":")) for sp in lines) + "\n ]\n}\n")
    print("%d specs, %d rows; branch hits: %s" % (len(lines), len(lines) * len(EMITS) * len(KNOBS), json.dumps(hits, sort_keys=True)), file=sys.stderr)


if __name__ == "__main__":
    main()
