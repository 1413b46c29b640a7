"""One table of the instantiations of the fp32 direct convolution (csrc/conv_mfma.hip, conv_mfma_kernel<KS, STRIDE, MREP, NREP, NW>): which
call, under which knobs, must run which one.  tests/test_mfma_coverage.py (CPU) holds the table to virnet_conv_mfma_tile and to the host's
dispatch list; tests/test_conv_mfma_gpu.py runs every row against an fp64 reference and against <KS, STRIDE, 1, 1> on the same tensors;
tests/test_redzone_mfma_gpu.py runs the rows of REDZONE between guard zones.

Why pinned: pick_tile gives every launch below 1024 four-row tiles ONE 32-channel slab per workgroup, eight-row tiles from 2048 and eight
waves from 512 tiles on, so a kernel-level test at a small shape runs <KS, STRIDE, 1, 1> and nothing else.  VIRNET_FORCE_MREP / _NREP / _NW
(read per call) pin the tile; `single` is the environment of the same call as <KS, STRIDE, 1, 1> with four waves.  Every instantiation
walks K in the same order per output element (chunk, tap, half-step, one fp32 MFMA chain), so the two must give the same bits.

kind: conv  3x3, stride 1 | 2, NHWC store (cin -> cout; stride 2: h, w are the INPUT's)
      convt the 2x2 stride-2 transposed conv = pointwise GEMM to 4 * cout rows + depth-to-space store (h, w: the input = the GEMM's grid)
      dgemm the transposed conv's input gradient (packing kind 3): pointwise GEMM, NHWC store; cin = the GEMM's contraction (4 x the
            forward layer's output channels), cout = its rows (the forward layer's input channels)
      planar 3x3, stride 1, planar store of cout <= 32 channels with crop; ops = (op, res_sf)
Shapes: the smallest with a partial tile on both axes whose last tile has one column, (TH + 1) x 33 outputs for TH = NW * MREP tile
rows, two images -- three where a row says so: 12 tiles, two per XCD, four workgroup slots that return early.  Planar rows:
(TH + 3) x 36 outputs cropped to (TH + 2) x 34.

Pure data: no device."""
from collections import namedtuple

Row = namedtuple("Row", "id kind ks stride transposed cin cout n h w ops env tile single seed")

# operand sets of the NHWC store (conv, dgemm) ...
#   plain: y_raw | act: y_act only | dual: both stores | bias_res: residual | mask_res: mask (slope 0.2) + residual
#   sft: both stores, per-image output mul / add | in_act: LeakyReLU on the input | in_sft: per-image in_mul / in_add + LeakyReLU
OPS = ("plain", "act", "dual", "bias_res", "mask_res", "sft", "in_act", "in_sft")
# ... of the transposed conv ...
T_OPS = ("bridge", "act", "dual", "mask")
# ... and of the planar store: (VIRNET_NCHW_* op, res_sf)
P_OPS = {"plain": ("plain", 1), "add": ("add", 1), "add_sf2": ("add", 2), "expclamp": ("expclamp", 1)}
CLAMP = (-0.5, 0.7)


def pin(mrep, nrep, nw):
    return {"VIRNET_CONV_FORM": "direct", "VIRNET_FORCE_MREP": str(mrep), "VIRNET_FORCE_NREP": str(nrep), "VIRNET_FORCE_NW": str(nw)}


SINGLE = pin(1, 1, 4)
# slabs per channel block in the packing (pick_nrep) of the channel counts the rows use
NREP_OF = {32: 1, 64: 2, 96: 3, 192: 3, 288: 3, 128: 4, 160: 5, 224: 7}
NREP_OF_T = {96: 3, 32: 4, 64: 4, 160: 4}                  # transposed: 4 * cout / 32 slabs
DEPTHS = (16, 32, 48)                                      # 1, 2, 3 chunks of the contraction

ROWS = []


def _add(kind, stride, cin, cout, ops, mrep, nw=4, n=2, nrep=None):
    """One row: the packed grouping of `cout` unless `nrep` = 1 asks for single slabs out of the wider packing."""
    ks = 3 if kind in ("conv", "planar") else 1
    packed = 1 if kind == "planar" else (NREP_OF_T if kind == "convt" else NREP_OF)[cout]
    nrep = packed if nrep is None else nrep
    th = nw * mrep
    if kind == "planar":
        h, w = th + 3, 36
    else:
        h, w = (th + 1) * stride, 33 * stride
    tag = {"conv": "", "convt": "t", "dgemm": "g", "planar": "p"}[kind]
    rid = f"k{ks}s{stride}{tag}-m{mrep}n{nrep}w{nw}-c{cin}to{cout}-{ops}" + ("-n3" if n == 3 else "")
    ROWS.append(Row(rid, kind, ks, stride, kind == "convt", cin, cout, n, h, w, ops, pin(mrep, nrep, nw), (ks, stride, mrep, nrep, nw), SINGLE,
                    100 + 10 * len(ROWS)))


def _all_ops(kind, stride, cout, mrep, nw=4, ops=OPS, **kw):
    for i, o in enumerate(ops):
        _add(kind, stride, DEPTHS[i % 3], cout, o, mrep, nw, **kw)


# ---- <3, 1, M, N>: every operand set on the three-slab workgroup at both tile heights; the other groupings once or twice each ------
_all_ops("conv", 1, 96, 1)
_all_ops("conv", 1, 96, 2)
_add("conv", 1, 16, 32, "plain", 1, n=3)
_add("conv", 1, 32, 32, "act", 2)
_add("conv", 1, 48, 96, "mask_res", 2, nrep=1)             # single slabs read out of the three-slab packing, eight-row tiles
_add("conv", 1, 32, 64, "dual", 1)
_add("conv", 1, 48, 64, "in_sft", 1)
_add("conv", 1, 16, 64, "mask_res", 2)
_add("conv", 1, 48, 64, "sft", 2, n=3)
_add("conv", 1, 32, 192, "sft", 1)                         # two channel blocks of three slabs
_add("conv", 1, 48, 192, "in_act", 2)
_add("conv", 1, 288, 288, "dual", 2)                       # 18 chunks, three channel blocks
_add("conv", 1, 16, 128, "bias_res", 1)
_add("conv", 1, 48, 128, "act", 1)
_add("conv", 1, 32, 160, "in_act", 1)
_add("conv", 1, 48, 160, "mask_res", 1)
_add("conv", 1, 16, 224, "act", 1)
_add("conv", 1, 224, 224, "plain", 1)                      # 14 chunks, seven slabs
# ---- <3, 2, 1, N> with 4 and with 8 waves ----------------------------------------------------------------------------------------
_all_ops("conv", 2, 96, 1)
_all_ops("conv", 2, 96, 1, nw=8)
_add("conv", 2, 16, 32, "plain", 1, n=3)
_add("conv", 2, 32, 64, "dual", 1)
_add("conv", 2, 48, 64, "act", 1, nw=8)
_add("conv", 2, 16, 64, "bias_res", 1, nw=8, n=3)
_add("conv", 2, 32, 192, "plain", 1, nw=8)
_add("conv", 2, 48, 288, "bias_res", 1)
_add("conv", 2, 32, 128, "mask_res", 1)
_add("conv", 2, 48, 128, "plain", 1)
_add("conv", 2, 16, 160, "sft", 1)
_add("conv", 2, 48, 160, "act", 1)
_add("conv", 2, 32, 224, "in_sft", 1)
_add("conv", 2, 48, 224, "dual", 1)
# ---- <1, 1, M, N>: the transposed conv (3 or 4 slabs) and the kind-3 GEMM (2, 3, 5, 7 slabs) ----------------------------------------
_all_ops("convt", 1, 96, 1, ops=T_OPS)
_all_ops("convt", 1, 96, 2, ops=T_OPS)
_add("convt", 1, 16, 96, "bridge", 2, nrep=1)              # <1,1,2,1>: one stage per launch, single slabs out of the three-slab packing
_add("convt", 1, 32, 96, "mask", 1, nrep=1)
_add("convt", 1, 16, 32, "bridge", 1, n=3)
_add("convt", 1, 48, 64, "act", 1)
_add("convt", 1, 32, 160, "dual", 1)
_add("convt", 1, 16, 160, "mask", 1)
_all_ops("dgemm", 1, 96, 2)
_all_ops("dgemm", 1, 64, 2)
_add("dgemm", 1, 16, 64, "plain", 1)                       # ONE stage: the weight ring's run-time slot arithmetic is the only path
_add("dgemm", 1, 48, 64, "mask_res", 1, n=3)
_add("dgemm", 1, 32, 96, "mask_res", 1)
_add("dgemm", 1, 16, 160, "dual", 1)
_add("dgemm", 1, 48, 160, "mask_res", 1)
_add("dgemm", 1, 16, 224, "in_sft", 1)
_add("dgemm", 1, 32, 224, "mask_res", 1)
# ---- planar store: the `n >= cout` skip and the crop are all that keeps these stores inside the buffer ---------------------------------
for _m in (1, 2):
    for _i, (_cout, _op) in enumerate([(1, "expclamp"), (3, "add_sf2"), (5, "add"), (17, "plain"), (32, "add")]):
        _add("planar", 1, DEPTHS[(_i + _m) % 3], _cout, _op, _m, n=3 if _cout == 5 else 2)

BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

CROP = lambda row: (row.h - 1, row.w - 2)                  # planar rows: smaller than the output on both axes, even (res_sf = 2)

# the rows of the red-zone module: per (KS, STRIDE, MREP, NW) the largest and the smallest NREP, and the planar rows with 5 and 32 channels
REDZONE = ["k3s1-m1n7w4-c224to224-plain", "k3s1-m1n1w4-c16to32-plain-n3", "k3s1-m2n3w4-c288to288-dual", "k3s1-m2n1w4-c48to96-mask_res",
           "k3s2-m1n7w4-c32to224-in_sft", "k3s2-m1n1w4-c16to32-plain-n3", "k3s2-m1n3w8-c48to96-sft", "k3s2-m1n2w8-c16to64-bias_res-n3",
           "k1s1g-m1n7w4-c16to224-in_sft", "k1s1g-m1n2w4-c16to64-plain", "k1s1t-m1n4w4-c16to32-bridge-n3", "k1s1t-m1n1w4-c32to96-mask",
           "k1s1t-m2n3w4-c16to96-bridge", "k1s1t-m2n1w4-c16to96-bridge", "k1s1g-m2n3w4-c32to96-mask_res",
           "k3s1p-m1n1w4-c16to5-add-n3", "k3s1p-m1n1w4-c48to32-add", "k3s1p-m2n1w4-c32to5-add-n3", "k3s1p-m2n1w4-c16to32-add"]
