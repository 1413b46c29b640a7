#!/usr/bin/env python
"""tests/golden/launch_plans.json: what the split-fp16 convolution hosts launch, RECORDED FROM THE COMMIT BEFORE conv_plan.h EXISTED.

The table is not produced by the code it tests.  Procedure (one-off, on a CPU-only machine):

  1. `python tests/golden/make_launch_plans.py specs > specs.txt` -- the curated rows below, one per line:
         family n h w cin_pad cout stride kind epi pre emit n_cu knobs     (knobs: `K=V,K=V` or `-`)
  2. In a scratch copy of the parent commit every launch template of conv_f16_wx4.hip / _wx4h / _wx4p / conv_f16.hip / _s2 / _pw was given
     the body `return record(form, rows, NG, NREP, variant, k.slab_base, k.NP / (32 * NG * NREP), persistent)` (variant: the direct kernel's
     MREP, the transposed conv's KS), conv_wx4_impl's `static int n_cu` was made settable, and a small driver called virnet_conv_wx4 /
     _wx4_emit / virnet_conv_f16 / _f16_emit / virnet_conv_bf16 / virnet_conv_f16_entry with the descriptor of each row (`desc_of` in
     tests/test_launch_plan.py states the same rule) and wrote `<spec> => <launch count> | <8 ints> | ...` or `<spec> => ERR <text>`.
     Rows with VIRNET_S2_WIDE=0 (read once per process) went through a driver process of their own.
  3. `python tests/golden/make_launch_plans.py json tests/golden/launch_plans_recorded.txt > tests/golden/launch_plans.json`
     (launch_plans_recorded.txt: the driver's output of step 2, committed as it was written)

The same driver ran an exhaustive grid (16.7 million rows: all four hosts x sizes x channel counts x epilogue / pre-activation classes x
emission x CU counts x knob settings, rejected descriptors included) through the recorder and through virnet_conv_plan_query: no difference.
"""
import json
import sys

WX4, F16, BF16, ENTRY = 0, 1, 2, 3          # the plan families as the recorded commit numbered them (a one-off recorder: nothing of the tree is imported)
NHWC, CONVT, PLANAR = 0, 1, 2                # kind
FIELDS = ("family", "n", "h", "w", "cin_pad", "cout", "stride", "kind", "epi", "pre", "emit", "n_cu")


def specs():
    rows = []

    def add(family, n, h, w, cin, cout, stride=1, kind=NHWC, epi=0, pre=0, emit=0, n_cu=256, knobs="-"):
        r = (family, n, h, w, cin, cout, stride, kind, epi, pre, emit, n_cu, knobs)
        if r not in rows:
            rows.append(r)

    def resblock(n, h, w, c, sft=False, knobs="-", n_cu=256, fams=(WX4, F16)):
        for fam in fams:
            add(fam, n, h, w, c, c, epi=0, pre=1, knobs=knobs, n_cu=n_cu)            # conv1: pre-activation, activated store
            add(fam, n, h, w, c, c, epi=1, pre=0, knobs=knobs, n_cu=n_cu)            # conv2: residual
            if sft:
                add(fam, n, h, w, c, c, epi=0, pre=2, knobs=knobs, n_cu=n_cu)        # SFT pre-activation (SISR)
                add(fam, n, h, w, c, c, epi=4, pre=1, knobs=knobs, n_cu=n_cu)        # SFT on the output / two stored tensors

    def unet(n, H, W, chans, sft=False):
        for lvl, c in enumerate(chans):
            h, w = H >> lvl, W >> lvl
            resblock(n, h, w, c, sft)
            if lvl + 1 < len(chans):
                add(F16, n, h, w, c, chans[lvl + 1], stride=2)                        # DownBlock.downsampler
                add(F16, n, h >> 1, w >> 1, chans[lvl + 1], c, kind=CONVT, epi=1)      # UpBlock.upsampler + bridge
        add(ENTRY, n, H, W, 16, chans[0])
        add(F16, n, H, W, 16, chans[0])
        add(F16, n, H, W, chans[0], 3, kind=PLANAR, epi=1)                            # tail + x_in
        for fam in (WX4, F16):                                                        # DnCNN (sigma net): 64 channels
            add(fam, n, H, W, 64, 64, pre=1)
        add(F16, n, H, W, 64, 3, kind=PLANAR)
        add(F16, n, H, W, 64, 6, kind=PLANAR)

    # every launch shape of tools/probes/rule_check.py (sizes padded to multiples of 4, three levels, conv1 / conv2, pinned tile heights)
    for H, W in ((256, 256), (128, 128), (484, 324), (500, 500)):
        for lvl, c in enumerate((96, 192, 288)):
            for knobs in ("-", "VIRNET_WX4_ROWS=8", "VIRNET_WX4_ROWS=16"):
                resblock(1, H >> lvl, W >> lvl, c, knobs=knobs, fams=(WX4,))
            resblock(1, H >> lvl, W >> lvl, c, fams=(F16,))
    # BASELINE configs 1..4 and the single-image cases of tools/bench_latency.py
    unet(64, 128, 128, (96, 192, 288))
    unet(32, 256, 256, (96, 192, 288))
    unet(1, 256, 256, (96, 160, 224), sft=True)
    unet(1, 512, 512, (96, 160, 224), sft=True)
    unet(4, 256, 256, (96, 192, 288))
    unet(1, 128, 128, (96, 192, 288))
    unet(1, 484, 324, (96, 192, 288))
    # configs[4]: the training step (T emission, mask epilogues of the input-gradient GEMMs, bf16 operands)
    for lvl, c in enumerate((96, 192, 288)):
        h = 128 >> lvl
        for emit in (8, 16):
            add(WX4, 32, h, h, c, c, epi=0, pre=1, emit=emit)
            add(WX4, 32, h, h, c, c, epi=1, pre=0, emit=emit)
        add(WX4, 32, h, h, c, c, epi=2)
        add(WX4, 32, h, h, c, c, epi=3)
        add(BF16, 32, h, h, c, c, epi=0, pre=1, emit=8)
        add(BF16, 32, h, h, c, c, epi=1)
        add(F16, 32, h, h, c, c, epi=2, emit=8)
    # tests/test_host.py::test_wx4_shape_rule
    for n, h, w, c in ((32, 256, 256, 96), (32, 128, 128, 192), (32, 64, 64, 288), (32, 256, 256, 64), (64, 32, 32, 288), (16, 64, 64, 224), (1, 256, 256, 96),
                       (1, 64, 64, 288), (1, 32, 32, 288), (1, 128, 128, 192), (1, 128, 128, 96), (1, 128, 128, 160), (32, 256, 256, 32), (64, 17, 33, 96), (1, 16, 32, 64)):
        for knobs in ("-", "VIRNET_WX4_MIN_WGS=0", "VIRNET_DETERMINISTIC=1"):
            add(WX4, n, h, w, c, c, pre=1, knobs=knobs)
        add(F16, n, h, w, c, c, pre=1)
    # thresholds (tools/knobs.md 2 and 4), a row on each side
    for h, w in ((256, 512), (128, 512), (112, 512), (128, 128), (120, 128)):                 # 128 workgroups of 96 channels / 192 single-slab workgroups
        resblock(1, h, w, 96, fams=(WX4, F16))
    for h in (128, 120):                                                                      # tiles8 * groups < n_cu: the launch leaves CUs empty
        for n_cu in (256, 304, 64):
            resblock(1, h, 256, 192, n_cu=n_cu, fams=(WX4,))
    for n, h in ((8, 256), (8, 240), (2, 256), (3, 256), (4, 256)):                # 8 rounds of 16-row workgroups, and the rounds below
        for c in (64, 96):
            add(WX4, n, h, 512, c, c, pre=1)
        add(WX4, n, h, 512, 96, 96, pre=1, n_cu=304)
    for h, w in ((128, 128), (256, 256), (256, 512), (512, 512)):                             # SFT table next to three slabs
        add(WX4, 1, h, w, 96, 96, pre=2)
        add(WX4, 1, h, w, 192, 192, pre=2)
    for c in (160, 224):                                                                      # five- and seven-slab channel counts
        for knobs in ("-", "VIRNET_WX4_WIDE=0", "VIRNET_WX4_ROWS=16", "VIRNET_WX4_ROWS=8", "VIRNET_WX4_NREP=1", "VIRNET_WX4_NREP=2", "VIRNET_WX4_NREP=3"):
            add(WX4, 16, 64, 64, c, c, pre=1, knobs=knobs)
            add(WX4, 1, 128, 128, c, c, pre=2, knobs=knobs)
        add(WX4, 16, 64, 64, c, c, pre=1, emit=8)
    for knobs in ("VIRNET_WX4_PERSIST=1", "VIRNET_WX4_PERSIST=1,VIRNET_WX4_PERSIST_MIN=0", "VIRNET_WX4_PERSIST=1,VIRNET_WX4_ROWS=8"):
        for n in (1, 4, 32):
            add(WX4, n, 256, 256, 96, 96, pre=1, knobs=knobs)
            add(WX4, n, 256, 256, 96, 96, pre=2, knobs=knobs)
        add(WX4, 32, 128, 128, 160, 160, epi=1, knobs=knobs)
        add(WX4, 32, 256, 256, 16, 96, knobs=knobs)
    for n, h in ((4, 256), (4, 248)):                                                         # direct kernel: 8-row tiles from 1024 workgroups on
        for knobs in ("-", "VIRNET_F16_MREP=1", "VIRNET_F16_MREP=2"):
            add(F16, n, h, 256, 96, 96, pre=1, knobs=knobs)
        add(F16, n, h, 256, 96, 3, kind=PLANAR, epi=1)
    for h, w, c in ((64, 64, 288), (64, 128, 288), (64, 96, 288), (128, 128, 160), (132, 128, 160), (64, 64, 160), (64, 64, 224), (256, 256, 160)):
        for knobs in ("-", "VIRNET_F16_SPLIT_WGS=0", "VIRNET_F16_SPLIT_WGS=512"):            # one slab per workgroup below 128 (mixed: 256) workgroups
            add(F16, 1, h, w, c, c, pre=1, knobs=knobs)
        add(F16, 1, h, w, c, c, pre=1, emit=8)
    for h, w in ((128, 128), (136, 256), (256, 256), (256, 384), (128, 256)):                # stride 2: 64 split tiles, 192 tiles x 6-slab groups
        for cout in (96, 128, 160, 192, 224, 288):
            add(F16, 1, h, w, 96, cout, stride=2)
        for knobs in ("VIRNET_S2_SPLIT_TILES=0", "VIRNET_S2_SPLIT_TILES=1000", "VIRNET_S2_WIDE=0"):
            add(F16, 1, h, w, 160, 224, stride=2, knobs=knobs)
            add(F16, 1, h, w, 192, 288, stride=2, knobs=knobs)
    for cin, cout in ((288, 192), (192, 96), (224, 160), (160, 96), (112, 64), (96, 192)):    # transposed: chunks per stage, slab groups
        for knobs in ("-", "VIRNET_CONVT_KS=3", "VIRNET_CONVT_SLABS=3", "VIRNET_CONVT_SLABS=2"):
            add(F16, 1, 64, 64, cin, cout, kind=CONVT, epi=1, knobs=knobs)
    # descriptors the hosts reject
    add(WX4, 1, 64, 64, 96, 80)
    add(WX4, 1, 64, 64, 24, 96)
    add(WX4, 1, 64, 64, 96, 96, stride=2)
    add(WX4, 1, 64, 64, 96, 96, epi=4, emit=8)
    add(WX4, 1, 64, 64, 16, 96, emit=16)
    add(F16, 1, 65, 64, 96, 96, stride=2)
    add(F16, 1, 64, 64, 96, 96, stride=2, epi=1)
    add(F16, 1, 64, 64, 96, 48, kind=PLANAR)
    add(F16, 1, 64, 64, 96, 96, kind=CONVT, epi=2)
    add(ENTRY, 1, 64, 64, 32, 96)
    add(ENTRY, 1, 64, 64, 16, 96, epi=1)
    add(BF16, 1, 64, 64, 96, 96, stride=2)
    return rows


def main():
    if sys.argv[1] == "specs":
        for r in specs():
            print(" ".join(str(v) for v in r))
        return
    want = [" ".join(str(v) for v in r) for r in specs()]
    got = {}
    for path in sys.argv[2:]:
        for line in open(path):
            spec, res = line.rstrip("\n").split(" => ", 1)
            got[spec] = res
    rows = []
    for spec in want:                                    # every curated row must have been recorded
        f = spec.split()
        res = got[spec]
        knobs = {} if f[12] == "-" else dict(kv.split("=") for kv in f[12].split(","))
        if res.startswith("ERR "):
            out = res[4:]
        else:
            parts = res.split(" | ")
            out = [[int(v) for v in p.split()] for p in parts[1:]]
            assert len(out) == int(parts[0])
        rows.append([int(v) for v in f[:12]] + [knobs, out])
    doc = {"fields": list(FIELDS) + ["knobs", "launches: [form, rows, ng, nrep, variant, slab_base, groups, persistent] each, or the error text"], "rows": rows}
    sys.stdout.write("{\n \"fields\": " + json.dumps(doc["fields"]) + ",\n \"rows\": [\n" +
                     ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
