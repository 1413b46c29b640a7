"""Red-zone runs of every kernel family (tests/redzone.py): the inputs, the weights, the packed images, the outputs and the workspaces
of each call sit between NaN-patterned guard zones, at the smallest shapes at which a tile walk can go wrong -- one partial tile on both
axes with the last image's last tile next to the zone, less than one tile, the degenerate 1 x 1 / 1 x w / h x 1, and the channel counts
of every slab grouping.  At these sizes the launch rules of csrc/conv_plan.h give every channel count ONE 32-channel slab per workgroup
(NREP = 1); the `*_slabs` forms pin the production groupings (3 / 3 + 2 / 3 + 2 + 2 / 2 slabs per workgroup), and the stride-2 and
transposed cases name the instantiation they reach.  Each case asserts
  (a) no zone was written, (b) its results live in guarded arenas, (c) every result element was written, (d) no result is NaN,
and that the guarded result is bit for bit the same call's result outside the guard (ops with floating-point atomics: their parity bar).
The workspace cache is cleared on entering the guard, so every scratch buffer is exactly as large as its size function says."""

import pytest
import torch

import redzone
from redzone import guarded
from virnet_amd import _native as nat
from virnet_amd import degrade, metrics, ops
from virnet_amd.networks import VIRAttResUNet, VIRAttResUNetSR
from virnet_amd.networks.AttResUNet import AttLayer
from virnet_amd.networks.KNet import KernelNet
from virnet_amd.utils.synth import synth_images, synth_state_dict
from test_ops_gpu import make_conv, nhwc, rnd
from test_sisr_train_gpu import SMALL

pytestmark = pytest.mark.gpu
PARITY = 2e-5          # tests/test_backward_gpu.py's bar, for the results that are sums of floating-point atomics

_WX4_OPEN = {"VIRNET_WX4_MIN_TILES": "0", "VIRNET_WX4_MIN_COUT": "0", "VIRNET_WX4_MIN_FILL": "0", "VIRNET_WX4_MIN_WGS": "0"}
# form id -> (environment, name the launch timer must report, tile rows the plan must report or None)
FORMS = {
    "direct": ({"VIRNET_CONV_FORM": "direct"}, "direct", None),
    "f16x3_m1": ({"VIRNET_CONV_FORM": "f16x3", "VIRNET_F16_MREP": "1"}, "f16x3", 4),
    "f16x3_m2": ({"VIRNET_CONV_FORM": "f16x3", "VIRNET_F16_MREP": "2"}, "f16x3", 8),
    "bf16": ({"VIRNET_CONV_FORM": "bf16"}, "bf16", None),
    "wino_nw4": ({"VIRNET_CONV_FORM": "wino", "VIRNET_WINO_NW": "4"}, "wino", None),
    "wino_nw8": ({"VIRNET_CONV_FORM": "wino", "VIRNET_WINO_NW": "8"}, "wino", None),
    "wx4_r16": (dict(_WX4_OPEN, VIRNET_CONV_FORM="wx4", VIRNET_WX4_ROWS="16"), "wx4", 16),
    "wx4_r8": (dict(_WX4_OPEN, VIRNET_CONV_FORM="wx4", VIRNET_WX4_ROWS="8"), "wx4", 8),
    # the multi-slab groupings, pinned (the entries above plan one slab per workgroup at the sizes of s1_cases)
    "f16x3_m1_slabs": ({"VIRNET_CONV_FORM": "f16x3", "VIRNET_F16_MREP": "1", "VIRNET_F16_SPLIT_WGS": "0"}, "f16x3", 4),
    "f16x3_m2_slabs": ({"VIRNET_CONV_FORM": "f16x3", "VIRNET_F16_MREP": "2", "VIRNET_F16_SPLIT_WGS": "0"}, "f16x3", 8),
    "wx4_r16_slabs": (dict(_WX4_OPEN, VIRNET_CONV_FORM="wx4", VIRNET_WX4_ROWS="16", VIRNET_WX4_NREP="3"), "wx4", 16),
    "wx4_r8_slabs": (dict(_WX4_OPEN, VIRNET_CONV_FORM="wx4", VIRNET_WX4_ROWS="8", VIRNET_WX4_NREP="3"), "wx4", 8),
}
ROWS = {"direct": 8, "f16x3_m1": 4, "f16x3_m2": 8, "bf16": 8, "wino_nw4": 8, "wino_nw8": 8, "wx4_r16": 16, "wx4_r8": 8,
        "f16x3_m1_slabs": 4, "f16x3_m2_slabs": 8, "wx4_r16_slabs": 16, "wx4_r8_slabs": 8}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("VIRNET_WINOGRAD", raising=False)
    monkeypatch.delenv("VIRNET_CONV_FORM", raising=False)
    monkeypatch.setenv("VIRNET_AUTOGRAPH", "0")            # eager launches: a captured graph would keep pointers into arenas that are gone


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class Launches:
    """What ran: the launch timer's keys, and the descriptor + form of every convolution (for virnet_conv_plan_query)."""

    def __enter__(self):
        self.timer, self.convs = ops.LaunchTimer(), []
        ops.set_launch_timer(self.timer)
        self._real = ops._launch_conv

        def spy(d, flops, what, form="direct", te=None):
            self.convs.append((d, form, te))
            return self._real(d, flops, what, form, te)
        ops._launch_conv = spy
        return self

    def __exit__(self, *exc):
        ops._launch_conv = self._real
        ops.set_launch_timer(None)
        return False

    def names(self):
        return ["direct" if isinstance(k[0], int) else k[0] for k in self.timer.summary()]

    def plans(self):
        fam = {"wx4": nat.PLAN_WX4, "f16x3": nat.PLAN_F16, "bf16": nat.PLAN_BF16}
        return [ops.conv_plan_query(fam[form], d, emit_rows=0 if te is None else te.rows) for d, form, te in self.convs if form in fam]

    def plan_rows(self):
        return [[l["rows"] for l in p] for p in self.plans()]

    def plan_slabs(self):
        """(wave groups, slabs per group, KS | MREP | 0) of every launch"""
        return [[(l["ng"], l["nrep"], l["variant"]) for l in p] for p in self.plans()]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def run_guarded(call, tensors, modules=(), *, allow_nan=False, bitwise=True, names=None, rows=None):
    """``call(**tensors)`` outside the guard, then inside it on ``guard_input`` copies with the parameters of ``modules`` moved into arenas
    and their weight images packed again; checks (a)-(d), then guarded == unguarded.  ``bitwise``: one flag, or one per result (False:
    PARITY relative to the largest element).  ``names`` / ``rows``: what the launch timer / the launch plans must report.
    Returns (guarded results, the Launches record)."""
    def flat(r):
        return [t for t in redzone._flatten(r)]
    plain = flat(call(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in tensors.items()}))      # (clones: `into=` accumulates in place)
    torch.cuda.synchronize()
    with guarded(modules) as g:
        for m in modules:
            g.adopt(m)
        inside = {k: (g.input(v) if isinstance(v, torch.Tensor) else v) for k, v in tensors.items()}
        with Launches() as rec:
            out = call(**inside)
            seen, planned = rec.names(), (rec.plan_rows() if rows is not None else None)
        got = flat(out)
        assert got, "the case returned no tensor"
        g.check(got, allow_nan=allow_nan)
        assert all(g.home(t) is not None for t in got)
    if names is not None:
        assert seen == names, seen
    if rows is not None:
        assert planned and all(r == rows for launch in planned for r in launch), planned
    assert len(got) == len(plain)
    flags = bitwise if isinstance(bitwise, (list, tuple)) else [bitwise] * len(got)
    for i, (a, b, bit) in enumerate(zip(got, plain, flags)):
        if bit:
            assert same_bits(a, b), (i, float((a.double() - b.double()).abs().max()))
        else:
            assert float((a - b).abs().max()) <= PARITY * max(float(b.abs().max()), 1e-12), i
    return out, rec


# ----------------------------------------------------------------------------------------------------------------------------------
# stride-1 3x3: every form x every epilogue set once x every shape class once
# ----------------------------------------------------------------------------------------------------------------------------------
def conv_case(cp, epi, n, c, cout, h, w, seed=1):
    """(call, tensors) of one conv_mfma epilogue set on NHWC tensors."""
    t = dict(x=nhwc(rnd(n, c, h, w, seed=seed)))
    if epi in ("res", "dual", "sft"):
        t["res"] = nhwc(rnd(n, cout, h, w, seed=seed + 1))
    if epi == "mask":
        t["mask"] = nhwc(rnd(n, cout, h, w, seed=seed + 2))
    if epi == "sft":
        t.update(in_mul=rnd(n, c, seed=seed + 3, lo=0.3, hi=1.0).cuda(), in_add=rnd(n, c, seed=seed + 4).cuda(),
                 mul=rnd(n, cout, seed=seed + 5, lo=0.3, hi=1.0).cuda(), add=rnd(n, cout, seed=seed + 6).cuda())
    kw = {"plain": dict(want_raw=True), "dual": dict(want_raw=True, want_act=True, slope=0.2), "res": dict(want_raw=True, in_slope=0.2),
          "mask": dict(want_raw=True, mask_slope=0.2), "sft": dict(want_raw=True, want_act=True, slope=0.2, in_slope=0.2),
          "preact": dict(want_raw=False, want_act=True, slope=0.25, in_slope=0.2)}[epi]

    def call(x, **more):
        return ops.conv_mfma(x, cp.packed(), **more, **kw)
    return call, t


def s1_cases(rows):
    # (shape class, channels, n, h, w, epilogue set)
    return [("partial_tile", 96, 2, rows + 1, 33, "plain"), ("sub_tile", 160, 1, 5, 7, "dual"), ("1x1", 192, 2, 1, 1, "res"),
            ("1xw", 224, 1, 1, 37, "mask"), ("hx1", 288, 1, rows + 1, 1, "sft"), ("sub_tile", 64, 3, 3, 2, "preact"),
            ("partial_tile", 32, 2, rows - 1, 31, "res")]


S1 = [(f, *case) for f in FORMS for case in s1_cases(ROWS[f])]


@pytest.mark.parametrize("form,cls,c,n,h,w,epi", S1, ids=[f"{s[0]}-{s[1]}-c{s[2]}-{s[6]}" for s in S1])
def test_stride1_conv(monkeypatch, form, cls, c, n, h, w, epi):
    env, name, rows = FORMS[form]
    setenv(monkeypatch, env)
    cp = make_conv(c, c, seed=80).cuda()
    call, t = conv_case(cp, epi, n, c, c, h, w)
    _, rec = run_guarded(call, t, [cp], names=[name], rows=rows)
    if name == "wx4":
        assert ops.wx4_last_plan()["rows"] == rows and not ops.wx4_last_plan()["persistent"]
    if form.endswith("_slabs"):                               # what the pinned grouping of c / 32 slabs is (conv_plan.h slab_groups)
        want = {1: [1], 2: [2], 3: [3], 5: [3, 2], 6: [3], 7: [3, 2], 9: [3]}[c // 32]
        assert rec.plan_slabs() == [[(1, nrep, 0 if name == "wx4" else rows // 4) for nrep in want]], rec.plan_slabs()


@pytest.mark.parametrize("c,n,h,w,wgs,epi", [(96, 2, 17, 33, 1, "plain"), (192, 1, 5, 7, 1, "preact"), (288, 2, 1, 1, 2, "res"), (96, 1, 1, 37, 1, "mask"),
                                             (96, 1, 17, 1, 1, "res"), (96, 3, 64, 96, 1, "res")])
def test_stride1_conv_wx4_persistent(monkeypatch, c, n, h, w, wgs, epi):
    """The persistent form (csrc/conv_f16_wx4p.hip); the last case has more items (36 tiles) than workgroups."""
    setenv(monkeypatch, dict(_WX4_OPEN, VIRNET_CONV_FORM="wx4", VIRNET_WX4_ROWS="16", VIRNET_WX4_NREP="3", VIRNET_WX4_PERSIST="1",
                             VIRNET_WX4_PERSIST_MIN="0", VIRNET_WX4_PERSIST_WGS=str(wgs)))
    cp = make_conv(c, c, seed=11).cuda()
    call, t = conv_case(cp, epi, n, c, c, h, w)
    run_guarded(call, t, [cp], names=["wx4"])
    assert ops.wx4_last_plan() == {"rows": 16, "persistent": True, "slabs": 3, "launches": 1}


# ---- dgrad packings: out_channels = the 32-padded rows (backward of thin layers), and the C -> C input-gradient GEMM -----------------
@pytest.mark.parametrize("form", ["direct", "wx4_r16"])
@pytest.mark.parametrize("cin,cout,n,h,w", [(4, 96, 2, 9, 33), (7, 64, 1, 5, 7), (3, 32, 2, 1, 1), (4, 96, 1, 1, 37), (3, 64, 2, 19, 1)])
def test_dgrad_conv_of_entry_layers(monkeypatch, form, cin, cout, n, h, w):
    """Input gradient of a forward cin -> cout entry layer (cin < 16): out_channels = the 32-padded rows.  Stored channels != the
    packing's rows, so ops.conv_form_rule keeps EVERY form on the fp32 direct kernel -- asserted, under the fp32 form and the default."""
    setenv(monkeypatch, FORMS[form][0])
    cp = make_conv(cin, cout, seed=90).cuda()
    run_guarded(lambda dy: ops.conv_mfma(dy, cp.packed_dgrad(), want_raw=True, out_channels=32), dict(dy=nhwc(rnd(n, cout, h, w, seed=91))), [cp],
                names=["direct"])


# what the input-gradient GEMM of an exit layer (forward 96 -> 3: a 16-channel gradient record in, one k-chunk) runs as: the packing has a
# split-fp16 image only (no Winograd images for a 16-channel contraction), so wx4 runs as f16x3 and wino as direct
_EXIT_DGRAD = {"direct": "direct", "f16x3_m2": "f16x3", "wx4_r16": "f16x3", "wino_nw4": "direct"}


@pytest.mark.parametrize("form", ["direct", "f16x3_m2", "wx4_r16", "wino_nw4"])
@pytest.mark.parametrize("cin,cout,n,h,w", [(96, 3, 1, 3, 34), (64, 1, 2, 1, 1), (96, 96, 2, 1, 35), (160, 160, 1, 9, 1), (96, 96, 2, 17, 33), (192, 192, 1, 3, 2)])
def test_dgrad_conv(monkeypatch, form, cin, cout, n, h, w):
    """Input-gradient GEMMs of a forward cin -> cout layer with the LeakyReLU mask and the residual: an exit layer's and the C -> C layers'."""
    env, name, rows = FORMS[form]
    setenv(monkeypatch, env)
    cp = make_conv(cin, cout, seed=90).cuda()
    thin = cout < 16
    t = dict(dy=nhwc(rnd(n, 16 if thin else cout, h, w, seed=91)), saved=nhwc(rnd(n, cin, h, w, seed=92)), skip=nhwc(rnd(n, cin, h, w, seed=93)))
    ran = _EXIT_DGRAD[form] if thin else name
    run_guarded(lambda dy, saved, skip: ops.conv_mfma(dy, cp.packed_dgrad(), mask=saved, mask_slope=0.2, res=skip, want_raw=True), t, [cp],
                names=[ran], rows=rows if ran == name and (form != "wx4_r16" or not thin) else None)
    if ran == "wx4":
        assert ops.wx4_last_plan()["rows"] == 16


# ---- stride-2 down conv: odd h/2, w/2; VIRNET_S2_SPLIT_TILES on both sides of its threshold -------------------------------------------
@pytest.mark.parametrize("form", ["direct", "f16x3_m2"])
@pytest.mark.parametrize("cin,cout,n,h,w,split", [(96, 192, 2, 10, 66, "0"), (96, 192, 2, 10, 66, "100000"), (160, 224, 1, 6, 14, "0"), (160, 224, 1, 6, 14, "100000"),
                                                  (64, 160, 2, 2, 2, "64"), (192, 288, 1, 2, 70, "64"), (96, 160, 1, 18, 2, "64"),
                                                  # the remaining instantiations of launch_f16_s2: wide 4 / wide 5 / <1,2>, and 192 tiles of 4 x 32 for <2,3> + <1,3>
                                                  (96, 128, 2, 10, 66, "0"), (96, 160, 2, 10, 66, "0"), (64, 64, 2, 10, 66, "0"), (48, 288, 6, 122, 66, "0")])
def test_stride2_conv(monkeypatch, form, cin, cout, n, h, w, split):
    """With the split off ("0") the cases reach <1,3> (96 -> 192), wide 7 (160 -> 224), wide 4, wide 5, <1,2> and <2,3> + <1,3>; the others
    run one slab per workgroup."""
    env, name, _ = FORMS[form]
    setenv(monkeypatch, dict(env, VIRNET_S2_SPLIT_TILES=split))
    cp = make_conv(cin, cout, stride=2, seed=9).cuda()

    def call(x):
        return ops.conv_mfma(x, cp.packed(), stride=2, want_raw=False, want_act=True)
    _, rec = run_guarded(call, dict(x=nhwc(rnd(n, cin, h, w, seed=9))), [cp], names=["direct" if form == "direct" else "f16x3_s2"])
    if form != "direct" and split == "0":
        want = {(96, 192): [(1, 3, 0)], (160, 224): [(1, 7, 0)], (96, 128): [(1, 4, 0)], (96, 160): [(1, 5, 0)], (64, 64): [(1, 2, 0)],
                (48, 288): [(2, 3, 0), (1, 3, 0)]}[(cin, cout)]
        assert rec.plan_slabs() == [want], rec.plan_slabs()


# ---- transposed 2x2: the 2h x 2w store ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["direct", "f16x3_m2"])
@pytest.mark.parametrize("cin,cout,n,h,w", [(192, 96, 2, 9, 33), (224, 160, 1, 5, 7), (288, 192, 2, 1, 1), (160, 96, 1, 1, 35), (64, 32, 3, 9, 1)])
def test_transposed_conv(monkeypatch, form, cin, cout, n, h, w):
    env, name, _ = FORMS[form]
    setenv(monkeypatch, env)
    cp = make_conv(cin, cout, ks=2, stride=2, transposed=True, seed=10).cuda()

    def call(x, bridge):
        return ops.conv_mfma(x, cp.packed(), res=bridge, want_raw=True, want_act=False)
    run_guarded(call, dict(x=nhwc(rnd(n, cin, h, w, seed=10)), bridge=nhwc(rnd(n, cout, 2 * h, 2 * w, seed=11))), [cp],
                names=["direct" if form == "direct" else "f16x3_t"])


@pytest.mark.parametrize("cin,cout,n,h,w,slabs,plan", [(96, 192, 2, 9, 33, "6", [(2, 3, 3)]), (192, 160, 1, 5, 7, "6", [(2, 3, 3), (1, 2, 3)]), (288, 64, 2, 1, 1, "3", [(1, 3, 3), (1, 2, 3)]),
                                                       (48, 32, 1, 1, 35, "6", [(1, 2, 3)]), (96, 32, 3, 9, 1, "6", [(1, 2, 3)])])
def test_transposed_conv_three_chunk_stages(monkeypatch, cin, cout, n, h, w, slabs, plan):
    """The KS = 3 pointwise kernels (VIRNET_CONVT_KS=3; 48 channels run them without the knob): the cases of test_transposed_conv plan KS = 2."""
    setenv(monkeypatch, dict(FORMS["f16x3_m2"][0], VIRNET_CONVT_KS="3", VIRNET_CONVT_SLABS=slabs))
    cp = make_conv(cin, cout, ks=2, stride=2, transposed=True, seed=10).cuda()

    def call(x, bridge):
        return ops.conv_mfma(x, cp.packed(), res=bridge, want_raw=True, want_act=False)
    _, rec = run_guarded(call, dict(x=nhwc(rnd(n, cin, h, w, seed=10)), bridge=nhwc(rnd(n, cout, 2 * h, 2 * w, seed=11))), [cp], names=["f16x3_t"])
    assert rec.plan_slabs() == [plan], rec.plan_slabs()


# ---- planar exits -----------------------------------------------------------------------------------------------------------------------
def exit_op(kind):
    if kind == "thin":
        return lambda x, cp, crop, **kw: ops.conv3x3_thin(x, cp.packed_thin(), crop, **kw)
    if kind == "mfma":
        return lambda x, cp, crop, **kw: ops.conv_mfma_nchw(x, cp.packed(), crop, **kw)
    return lambda x, cp, crop, **kw: ops.conv_f16_nchw(x, cp.packed(), crop, **kw)


EXITS = {"exit_rows": ({"VIRNET_CONV_FORM": "wx4", "VIRNET_EXIT_FORM": "rows"}, "exit"), "exit_f16": ({"VIRNET_CONV_FORM": "wx4", "VIRNET_EXIT_FORM": "f16"}, "f16x3"),
         "thin": ({"VIRNET_CONV_FORM": "direct"}, "thin"), "mfma": ({"VIRNET_CONV_FORM": "direct"}, "direct")}
# (cout, c, n, h, w, crop, mode): crop = full | less (h-3, w-1) | one (1 x 1); mode = plain | add | add_sf2 | expclamp
EXIT_CASES = [(3, 96, 2, 9, 33, "full", "add"), (1, 64, 1, 5, 7, "less", "expclamp"), (2, 160, 2, 17, 34, "one", "plain"), (3, 96, 1, 8, 34, "full", "add_sf2"),
              (4, 96, 2, 7, 31, "less", "add"), (3, 64, 2, 1, 1, "full", "plain"), (1, 96, 1, 1, 37, "one", "add"), (2, 64, 1, 19, 1, "full", "expclamp")]


@pytest.mark.parametrize("kind", list(EXITS))
@pytest.mark.parametrize("cout,c,n,h,w,crop,mode", EXIT_CASES)
def test_planar_exit(monkeypatch, kind, cout, c, n, h, w, crop, mode):
    env, name = EXITS[kind]
    setenv(monkeypatch, env)
    if kind == "exit_rows" and cout > 3:
        name = "f16x3"                                            # (more than 3 channels have no taps-as-rows image: conv_f16's planar form)
    cp = make_conv(c, cout, seed=50).cuda()
    ch, cw = {"full": (h, w), "less": (max(h - 3, 1), max(w - 1, 1)), "one": (1, 1)}[crop]
    op = exit_op(kind)
    t = dict(x=nhwc(rnd(n, c, h, w, seed=50)))
    kw = {}
    if mode == "add":
        t["res"], kw = rnd(n, cout, ch, cw, seed=51).cuda(), dict(op=nat.NCHW_ADD)
    elif mode == "add_sf2":
        t["res"], kw = rnd(n, cout, ch // 2, cw // 2, seed=52).cuda(), dict(op=nat.NCHW_ADD, res_sf=2)
    elif mode == "expclamp":
        kw = dict(op=nat.NCHW_EXPCLAMP, clamp=(-0.5, 0.7))
    run_guarded(lambda x, res=None: op(x, cp, (ch, cw), res=res, **kw), t, [cp], names=[name])


# ---- entry ---------------------------------------------------------------------------------------------------------------------------------
# n, c0, h, w, sf, hp, wp, ev, em, msf, map_sqrt, cout
ENTRY = [(2, 3, 9, 33, 1, 12, 36, 0, 1, 1, True, 96),        # image + sqrt(map); the pad at its limit (hp - h = 3)
         (1, 3, 5, 7, 2, 12, 16, 3, 0, 1, False, 64),        # nearest x2 + vector
         (2, 3, 3, 5, 3, 12, 16, 3, 1, 3, True, 96),         # nearest x3 + vector + low-resolution map; pad 3 = the limit
         (3, 1, 4, 4, 1, 4, 4, 0, 2, 1, False, 32),          # no pad, one image channel, two map channels
         (1, 3, 17, 4, 1, 20, 4, 0, 1, 1, True, 96),         # pad on one axis only
         (2, 3, 1, 1, 1, 1, 1, 0, 1, 1, True, 96),           # 1 x 1, no pad: every halo pixel is outside the image
         (1, 3, 1, 37, 1, 1, 40, 0, 1, 1, True, 64),         # 1 x w, reflect pad along w only
         (2, 3, 19, 1, 1, 20, 1, 3, 0, 1, False, 96),        # h x 1, reflect pad along h only
         (1, 3, 1, 1, 3, 4, 4, 3, 1, 3, True, 96)]           # a 1 x 1 image, nearest x3 -> 3 x 3, reflect-padded to 4 x 4 (1 x 1 map)
ENTRY_FORMS = {"pack_input": {}, "conv_entry": {"VIRNET_CONV_FORM": "wx4"}, "conv_f16_entry": {"VIRNET_CONV_FORM": "wx4", "VIRNET_ENTRY_FORM": "f16"}}


def entry_tensors(n, c0, h, w, sf, ev, em, msf):
    return dict(x=rnd(n, c0, h, w, seed=62, lo=0.0, hi=1.0).cuda(), vec=rnd(n, ev, seed=63).cuda() if ev else None,
                map_=rnd(n, em, h * sf // msf, w * sf // msf, seed=64, lo=0.01, hi=2.0).cuda() if em else None)


@pytest.mark.parametrize("which", list(ENTRY_FORMS))
@pytest.mark.parametrize("n,c0,h,w,sf,hp,wp,ev,em,msf,msqrt,cout", ENTRY)
def test_entry(monkeypatch, which, n, c0, h, w, sf, hp, wp, ev, em, msf, msqrt, cout):
    setenv(monkeypatch, ENTRY_FORMS[which])
    t = entry_tensors(n, c0, h, w, sf, ev, em, msf)
    if which == "pack_input":
        for zero_pad in (False, True):
            run_guarded(lambda x, vec, map_: ops.pack_input(x, hp, wp, sf=sf, vec=vec, map_=map_, map_sf=msf, map_sqrt=msqrt, zero_pad=zero_pad), t)
        return
    cp = make_conv(c0 + ev + em, cout, seed=61).cuda()
    run_guarded(lambda x, vec, map_: ops.conv_entry(x, cp.packed(), hp, wp, sf=sf, vec=vec, map_=map_, map_sf=msf, map_sqrt=msqrt, want_act=cout == 64, slope=0.25),
                t, [cp], names=["entry" if which == "conv_entry" else "f16x3"])


@pytest.mark.parametrize("which", list(ENTRY_FORMS))
@pytest.mark.parametrize("h,w,hp,wp", [(2, 2, 4, 4), (1, 1, 4, 4), (1, 5, 4, 8), (5, 1, 8, 1 + 1)])
def test_entry_rejects_a_pad_as_large_as_the_image_and_touches_nothing(monkeypatch, which, h, w, hp, wp):
    """2 x 2 -> 4 x 4, and a one-pixel axis with any pad at all: the reflect pad's contract (pad < dim) refuses it; the zones stay clean."""
    setenv(monkeypatch, ENTRY_FORMS[which])
    cp = make_conv(3, 64, seed=61).cuda()
    with guarded([cp]) as g:
        g.adopt(cp)
        x = g.input(rnd(2, 3, h, w, seed=1).cuda())
        with pytest.raises(RuntimeError):
            if which == "pack_input":
                ops.pack_input(x, hp, wp)
            else:
                ops.conv_entry(x, cp.packed(), hp, wp)
        assert g.arenas and not g.zone_findings()


# ---- T emission: the T image and the column partials at exactly their *_bytes sizes ---------------------------------------------------------
T_CASES = [(f, r, *s) for f, r in (("f16x3", 0), ("bf16", 0), ("wx4", 16)) for s in ((2, 9, 9, 96), (1, 5, 32, 160), (2, 17, 37, 64),
                                                                                          (2, 1, 1, 96), (1, 1, 37, 64), (1, 19, 1, 96), (3, 3, 2, 160))]
T_CASES.append(("wx4", 8, 3, 70, 70, 288))        # the 8-row emitting form runs from 128 16-row workgroups on only: 3 x 5 x 3 tiles x 3 channel blocks


@pytest.mark.parametrize("form,rows,n,h,w,c", T_CASES)
def test_t_emission(monkeypatch, form, rows, n, h, w, c):
    setenv(monkeypatch, dict(_WX4_OPEN, VIRNET_CONV_FORM=form))
    if rows == 16:
        setenv(monkeypatch, {"VIRNET_WX4_ROWS": "16", "VIRNET_WX4_EMIT_ROWS": "16"})
    elif rows == 8:
        setenv(monkeypatch, {"VIRNET_WX4_MIN_WGS": "1", "VIRNET_WX4_EMIT_ROWS": "8"})
    cp = make_conv(c, c, seed=31).cuda()
    lib = nat.load()
    held = []

    def call(x, res):
        raw, _, timg = ops.conv_mfma(x, cp.packed(), res=res, in_slope=0.2, want_raw=True, emit=dict(act=0.2, colsum=c))
        assert timg is not None and (timg.n, timg.h, timg.w, timg.c) == (n, h, w, c)
        assert timg.buf.numel() == lib.virnet_chsplit_bytes(n, h, w, c) and timg.col.numel() == timg.nblk * c * 4
        held.append(timg.col)
        return raw, timg.buf, timg.bias_sums()
    with guarded([cp]) as g:
        g.adopt(cp)
        with Launches() as rec:
            raw, buf, db = call(g.input(nhwc(rnd(n, c, h, w, seed=32))), g.input(nhwc(rnd(n, c, h, w, seed=33))))
            seen = rec.names()
        assert g.home(buf) is not None and g.home(buf).nbytes == buf.numel()              # the arena is exactly chsplit_bytes: its zones start there
        assert g.home(held[0]) is not None and g.home(held[0]).nbytes == held[0].numel()  # and the column partials' exactly nblk * c * 4
        g.check([raw, db])
        g.check([buf], allow_nan=True)                                                     # (bytes: only home + zones apply)
    assert seen == [form]
    plain = call(nhwc(rnd(n, c, h, w, seed=32)), nhwc(rnd(n, c, h, w, seed=33)))
    assert same_bits(raw, plain[0]) and same_bits(buf, plain[1])
    assert float((db - plain[2]).abs().max()) <= PARITY * float(plain[2].abs().max())


# ---- weight gradients -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wform", ["f16", "f32"])
@pytest.mark.parametrize("cin,cout,n,h,w", [(96, 96, 2, 5, 33), (160, 64, 1, 6, 9), (32, 288, 2, 7, 65), (224, 16, 1, 5, 37), (16, 96, 2, 9, 31)])
def test_conv_wgrad(monkeypatch, wform, cin, cout, n, h, w):
    """f16: chsplit x 2 (+ column partials) + conv_wgrad_f16 with wgrad_xt / wgrad_yt / wgrad_col / wgrad_part at their declared sizes;
    f32: the fp32 split-K kernel (atomics: parity bar) + colsum with cvalid < c."""
    setenv(monkeypatch, {"VIRNET_CONV_FORM": "wx4", "VIRNET_WGRAD_FORM": wform})
    real_cout = 3 if cout == 16 else cout
    real_cin = 4 if cin == 16 else cin
    t = dict(x=nhwc(rnd(n, cin, h, w, seed=310)), dy=nhwc(rnd(n, cout, h, w, seed=311)),
             in_mul=rnd(n, cin, seed=312, lo=0.3, hi=1.0).cuda(), in_add=rnd(n, cin, seed=313).cuda())

    def call(x, dy, in_mul, in_add):
        return ops.conv_wgrad(x, dy, (real_cout, real_cin, 3, 3), in_slope=0.2, in_mul=in_mul, in_add=in_add, bias_channels=real_cout)
    _, rec = run_guarded(call, t, bitwise=[wform == "f16", False], names=["wgrad_f16" if wform == "f16" else "wgrad"])


@pytest.mark.parametrize("cin,cout,n,oh,ow", [(96, 192, 2, 5, 33), (160, 224, 1, 6, 9), (64, 96, 2, 7, 3)])
def test_stride2_and_transposed_wgrad(monkeypatch, cin, cout, n, oh, ow):
    """chsplit_s2 + chsplit + conv_wgrad_f16_s2 (both modes) and, with VIRNET_WGRAD_FORM=f32, the fp32 kernel on space_to_depth2."""
    setenv(monkeypatch, {"VIRNET_CONV_FORM": "wx4"})
    hi, lo = nhwc(rnd(n, cin, 2 * oh, 2 * ow, seed=320)), nhwc(rnd(n, cout, oh, ow, seed=321))
    run_guarded(lambda x, dy: ops.conv_wgrad(x, dy, (cout, cin, 3, 3), stride=2, in_slope=0.2, bias_channels=cout), dict(x=hi, dy=lo),
                bitwise=[True, False], names=["wgrad_f16_s2"])
    # transposed conv cout -> cin: its input is the low-resolution tensor, dy the high-resolution one
    run_guarded(lambda x, dy: ops.convt_wgrad(x, dy, (cout, cin, 2, 2)), dict(x=lo, dy=hi), bitwise=[True, False], names=["wgrad_f16_s2"])
    monkeypatch.setenv("VIRNET_WGRAD_FORM", "f32")
    run_guarded(lambda x, dy: ops.conv_wgrad(x, dy, (cout, cin, 3, 3), stride=2, bias_channels=cout), dict(x=hi, dy=lo), bitwise=False, names=["wgrad"])
    run_guarded(lambda x, dy: ops.convt_wgrad(x, dy, (cout, cin, 2, 2)), dict(x=lo, dy=hi), bitwise=False, names=["wgrad"])


SMALL_MAPS = [(1, 1), (1, 37), (9, 1), (3, 2), (4, 33)]


@pytest.mark.parametrize("wform", ["f16", "f32"])
@pytest.mark.parametrize("h,w", SMALL_MAPS)
@pytest.mark.parametrize("cin,cout", [(96, 96), (64, 160)])
def test_conv_wgrad_small_maps(monkeypatch, wform, cin, cout, h, w):
    """1 x 1, 1 x w, h x 1 and sub-tile maps.  Below five rows the f16 path's row ring does not apply and ops.conv_wgrad takes the fp32
    split-K kernel with its tile counters (what the deepest levels run at small patches), whatever VIRNET_WGRAD_FORM says -- asserted."""
    setenv(monkeypatch, {"VIRNET_CONV_FORM": "wx4", "VIRNET_WGRAD_FORM": wform})
    n = 2
    t = dict(x=nhwc(rnd(n, cin, h, w, seed=340)), dy=nhwc(rnd(n, cout, h, w, seed=341)))
    f16 = wform == "f16" and h >= 5
    run_guarded(lambda x, dy: ops.conv_wgrad(x, dy, (cout, cin, 3, 3), in_slope=0.2, bias_channels=cout), t,
                bitwise=[f16, False], names=["wgrad_f16" if f16 else "wgrad"])


@pytest.mark.parametrize("wform", ["f16", "f32"])
@pytest.mark.parametrize("oh,ow", SMALL_MAPS)
def test_stride2_and_transposed_wgrad_small_maps(monkeypatch, wform, oh, ow):
    """The same for the stride-2 conv (output oh x ow) and the transposed conv (input oh x ow): below five low-resolution rows both run the
    fp32 kernel, convt_wgrad on space_to_depth2 of its gradient plus colsum."""
    setenv(monkeypatch, {"VIRNET_CONV_FORM": "wx4", "VIRNET_WGRAD_FORM": wform})
    n, cin, cout = 2, 96, 160
    hi, lo = nhwc(rnd(n, cin, 2 * oh, 2 * ow, seed=350)), nhwc(rnd(n, cout, oh, ow, seed=351))
    f16 = wform == "f16" and oh >= 5
    name = ["wgrad_f16_s2" if f16 else "wgrad"]
    run_guarded(lambda x, dy: ops.conv_wgrad(x, dy, (cout, cin, 3, 3), stride=2, in_slope=0.2, bias_channels=cout), dict(x=hi, dy=lo),
                bitwise=[f16, False], names=name)
    run_guarded(lambda x, dy: ops.convt_wgrad(x, dy, (cout, cin, 2, 2)), dict(x=lo, dy=hi), bitwise=[f16, False], names=name)


@pytest.mark.parametrize("n,h,w", [(2, 9, 7), (1, 21, 30), (1, 1, 1)])
def test_head_s4_conv_and_gradients(n, h, w):
    x, wt = rnd(n, 3, h, w, seed=22, lo=0, hi=1).cuda(), (rnd(64, 3, 9, 9, seed=21) * 0.06).cuda()
    (out,), _ = run_guarded(lambda x, wt: (ops.conv_head_s4(x, wt),), dict(x=x, wt=wt))
    dy = torch.from_numpy(rnd(*out.shape, seed=23).numpy()).cuda()
    run_guarded(lambda dy, wt: ops.conv_head_s4_dgrad(dy, wt, (h, w)), dict(dy=dy, wt=wt))
    run_guarded(lambda x, dy: ops.conv_head_s4_wgrad(x, dy, 64), dict(x=x, dy=dy), bitwise=False)


@pytest.mark.parametrize("c,cvalid,npix", [(96, 96, 35), (16, 3, 1), (160, 130, 577)])
def test_colsum_and_colpart_reduce(c, cvalid, npix):
    dy = rnd(1, npix, 1, c, seed=330).cuda()
    run_guarded(lambda dy: ops.colsum(dy, cvalid), dict(dy=dy), bitwise=False)
    if c % 32 == 0:
        nblk = 5
        col = rnd(c // 32 * nblk * 32, seed=331).cuda()

        def call(col):
            t = ops.TImage(None, 1, 1, 1, c, False, col=col, nblk=nblk, ncol=cvalid)
            return t.bias_sums()
        run_guarded(call, dict(col=col))


# ---- small kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,h,w", [(2, 96, 9, 33), (1, 160, 5, 7), (3, 64, 1, 1), (1, 288, 1, 37)])
def test_layout_and_sft_backward_kernels(n, c, h, w):
    t = dict(da=nhwc(rnd(n, c, h, w, seed=1)), x=nhwc(rnd(n, c, h, w, seed=2)), mul=rnd(n, c, seed=3, lo=0.3, hi=1.0).cuda(), add=rnd(n, c, seed=4).cuda(),
             res=nhwc(rnd(n, c, h, w, seed=5)))
    run_guarded(lambda da, x, mul, add, res: ops.sft_backward(da, x, mul, add, slope=0.2, res=res), t, bitwise=[True, False, False])
    run_guarded(lambda dy: ops.zero_stuff2(dy), dict(dy=t["x"]))
    run_guarded(lambda dy: ops.space_to_depth2(dy), dict(dy=nhwc(rnd(n, c, 2 * h, 2 * w, seed=6))))


@pytest.mark.parametrize("n,h,w,hp,wp,sqrt", [(2, 37, 45, 40, 48, True), (1, 5, 7, 8, 8, False), (2, 4, 4, 4, 4, True)])
def test_pack_input_backward(n, h, w, hp, wp, sqrt):
    g, sig = rnd(n, hp, wp, 16, seed=7).cuda(), rnd(n, 1, h, w, seed=8, lo=0.1, hi=2).cuda()
    run_guarded(lambda drec, sig: ops.pack_input_backward(drec, 3, (h, w), map_=sig, map_sqrt=sqrt), dict(drec=g, sig=sig))
    run_guarded(lambda drec, sig, acc: ops.pack_input_backward(drec, 3, (h, w), map_=sig, map_sqrt=sqrt, into=acc),
                dict(drec=g, sig=sig, acc=rnd(n, 1, h, w, seed=9).cuda()))


def _ceil(v, m):
    return (v + m - 1) // m * m


@pytest.mark.parametrize("sf,c0,cf,n,h,w,terms", [(1, 3, 96, 2, 21, 19, "abr"), (1, 1, 64, 2, 9, 7, "abr"), (2, 3, 64, 2, 9, 7, "ar"), (3, 1, 96, 1, 9, 7, "ar"),
                                                  (4, 3, 64, 1, 9, 7, "ar"), (4, 1, 96, 2, 21, 19, "a"), (2, 3, 96, 1, 21, 19, "r"), (1, 3, 64, 1, 21, 19, "b"),
                                                  (1, 1, 96, 1, 33, 5, "ab"), (3, 3, 64, 1, 21, 19, "abr+"), (1, 3, 96, 2, 9, 7, "a+")])
def test_image_grad(sf, c0, cf, n, h, w, terms):
    """Every term set of tests/test_input_grad_gpu.py (its one workload-sized shape replaced by a small ragged one)."""
    H, W = h * sf, w * sf
    hp, wp = _ceil(H, 8), _ceil(W, 8)
    t = dict(dres=rnd(n, c0, H, W, seed=6).cuda() if "r" in terms else None,
             ga=nhwc(rnd(n, cf, hp, wp, seed=4)) if "a" in terms else None, wa=(rnd(cf, c0 + 2, 3, 3, seed=2) * 0.2).cuda() if "a" in terms else None,
             gb=nhwc(rnd(n, 64, h, w, seed=5)) if "b" in terms else None, wb=(rnd(64, c0, 3, 3, seed=3) * 0.2).cuda() if "b" in terms else None,
             into=torch.ones(n, c0, h, w, device="cuda") if "+" in terms else None)
    run_guarded(lambda **kw: ops.image_grad((h, w), c0, n=n, sf=sf, **kw), t)


@pytest.mark.parametrize("n,c,h,w", [(3, 3, 7, 9), (2, 2, 33, 31), (1, 5, 1, 1), (2, 3, 1, 67)])
def test_gap_nchw(n, c, h, w):
    x = rnd(n, c, h, w, seed=29, lo=-12, hi=3).cuda()
    for finish, clamp in ((ops.GAP_MEAN, (0.0, 0.0)), (ops.GAP_EXPCLAMP, (-1.0, 1.0)), (ops.GAP_KINFO, (-6.0, 2.0))):
        if finish == ops.GAP_KINFO and c != 3:
            continue
        run_guarded(lambda x: ops.gap_nchw(x, finish, clamp), dict(x=x))


@pytest.mark.parametrize("n,h,w", [(2, 31, 33), (3, 65, 64), (2, 1, 1), (1, 5, 7)])
def test_calayer_kernels(n, h, w):
    """ca_gate + scale_add and the fused ca_scale_add on both sides of its one-launch limit (64 x 64 x 64 / 4 items)."""
    t = dict(hcv=nhwc(rnd(n, 64, h, w, seed=23)), skip=nhwc(rnd(n, 64, h, w, seed=24)), w1=(rnd(4, 64, 1, 1, seed=25) * 0.2).cuda(), b1=(rnd(4, seed=26) * 0.1).cuda(),
             w2=rnd(64, 4, 1, 1, seed=27).cuda(), b2=(rnd(64, seed=28) * 0.1).cuda())
    run_guarded(lambda hcv, skip, w1, b1, w2, b2: ops.scale_add(hcv, ops.ca_gate(hcv, w1, b1, w2, b2), skip), t)
    run_guarded(lambda hcv, skip, w1, b1, w2, b2: ops.ca_scale_add(hcv, w1, b1, w2, b2, skip), t)


def _knet(blocks, seed=7):
    knet = KernelNet(3, 3, num_blocks=blocks)
    knet.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in knet.state_dict().items()}, seed=seed))
    return knet.cuda().eval()


@pytest.mark.parametrize("blocks,shape", [(3, (2, 3, 21, 30)), (2, (2, 3, 4, 61)), (9, (2, 3, 33, 64)), (2, (1, 3, 1, 1))])
def test_knet_body(monkeypatch, blocks, shape):
    """The persistent KernelNet body (one workgroup per image walks every layer; the nine-layer case is more than one launch holds)
    through KernelNet.forward.  The two recorded calls are the unguarded and the guarded forward: both took the persistent route."""
    setenv(monkeypatch, {"VIRNET_CONV_FORM": "wx4", "VIRNET_KNET_PERSISTENT": "1"})
    knet = _knet(blocks)
    calls = []
    real = ops.knet_body
    monkeypatch.setattr(ops, "knet_body", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def call(x):
        with torch.no_grad():
            return knet(x)
    run_guarded(call, dict(x=synth_images(*shape, seed=3).cuda()), [knet])
    assert len(calls) == 2


@pytest.mark.parametrize("nf,e,n", [(96, 4, 3), (160, 4, 1), (224, 4, 2), (64, 1, 2)])
def test_sft_generators(nf, e, n):
    torch.manual_seed(31)
    att = AttLayer(nf, e).cuda()
    run_guarded(lambda vec: ops.sft_vec(vec, att), dict(vec=rnd(n, e, seed=31, lo=0, hi=1.5).cuda()), [att])
    H, W = 6, 10
    rec = torch.zeros(n, H, W, 16)
    rec[..., :3 + e] = rnd(n, H, W, 3 + e, seed=32, lo=0, hi=1)
    run_guarded(lambda raw, rec: ops.sft_apply(raw, rec, 3, e, 2, att), dict(raw=nhwc(rnd(n, nf, H // 2, W // 2, seed=33)), rec=rec.cuda()), [att])
    run_guarded(lambda raw, rec: ops.sft_apply(raw, rec, 3, e, 1, att), dict(raw=nhwc(rnd(n, nf, H, W, seed=34)), rec=rec.cuda()), [att])


def test_sft_vec_multi_two_launches():
    torch.manual_seed(34)
    atts = torch.nn.ModuleList([AttLayer(nf, 4) for nf in (96, 96, 160, 160, 224, 224) * 3]).cuda()      # 18 layers: 16 + 2
    run_guarded(lambda vec: ops.sft_vec_multi(vec, list(atts)), dict(vec=rnd(3, 4, seed=35, lo=0, hi=1.5).cuda()), [atts])


@pytest.mark.parametrize("numel", [1, 7, 1023, 4098 + 3])
@pytest.mark.parametrize("up", [0, 1])
def test_poison_on_flag(numel, up):
    """n not a multiple of 4 (the kernel stores float4 groups): flag clear -> y untouched; flag up -> all NaN, nothing beyond y."""
    y = rnd(numel, seed=40).cuda()

    def call(flag, y):
        ops.poison_on_flag(flag, y)
        return y
    (out,), _ = run_guarded(lambda flag, y: (call(flag, y),), dict(flag=torch.full((1,), up, dtype=torch.int32, device="cuda"), y=y.clone()), allow_nan=True)
    assert bool(torch.isnan(out).all()) if up else same_bits(out, y)


# ---- metrics and degradation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 12, 37), (1, 1, 1, 5), (3, 3, 5, 7), (1, 3, 1, 1023)])
def test_quantise_and_luma(shape):
    x = (rnd(*shape, seed=50) * 0.8 + 0.5).cuda()
    (u8,), _ = run_guarded(lambda x: (metrics.to_uint8(x),), dict(x=x))
    if shape[1] == 3:
        run_guarded(lambda u: metrics.rgb2y(u), dict(u=u8.clone()))


@pytest.mark.parametrize("ycbcr", [False, True], ids=["rgb", "y"])
@pytest.mark.parametrize("border", [0, 4])
@pytest.mark.parametrize("n,h,w,as_float", [(2, 19, 37, False), (1, 23, 70, True), (3, 11 + 8, 11 + 8, False)])
def test_psnr_ssim(border, ycbcr, n, h, w, as_float):
    """Widths that are no multiple of the SSIM tile, the smallest image border 4 leaves an 11 x 11 window in; the int64 workspace is
    exactly virnet_psnr_ssim_workspace_bytes."""
    a = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(51)).cuda()
    b = (a.float() + torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(52)).cuda() * 12).clamp(0, 255).to(torch.uint8)
    if as_float:
        a = a.float() / 255.0
    run_guarded(lambda a, b: metrics.psnr_ssim(a, b, border=border, ycbcr=ycbcr), dict(a=a, b=b))


DEGRADE_SHAPES = {"fold_both_sides": (2, 3, 12, 15, 21), "pad_limit": (1, 1, 11, 11, 21), "ceil_sizes": (2, 3, 44, 52, 21)}


@pytest.mark.parametrize("down,sf", [("direct", 3), ("bicubic", 4), ("direct", 1)])
@pytest.mark.parametrize("border", ["reflect", "symmetric"])
@pytest.mark.parametrize("name", list(DEGRADE_SHAPES))
def test_degrade_forward_and_adjoints(name, border, down, sf):
    """blur_downsample forward, image adjoint and kernel adjoint (its workspace exactly virnet_degrade_grad_kernel_workspace_bytes), through
    autograd as the product calls them; the bicubic path runs resample_axis in both directions and both precisions."""
    n, c, h, w, k = DEGRADE_SHAPES[name]
    g = torch.Generator().manual_seed(6)
    x, ker = torch.rand(n, c, h, w, generator=g).cuda(), torch.rand(n, 1, k, k, generator=g).cuda()
    ker = ker / ker.sum((2, 3), keepdim=True)
    gy = torch.randn(n, c, -(-h // sf), -(-w // sf), generator=g).cuda()

    def call(x, ker, gy):
        x, ker = x.detach().requires_grad_(True), ker.detach().requires_grad_(True)
        y = degrade.blur_downsample(x, ker, sf, down, border)
        gx, gk = torch.autograd.grad(y, [x, ker], gy)
        return y.detach(), gx, gk
    run_guarded(call, dict(x=x, ker=ker, gy=gy))


@pytest.mark.parametrize("n_in,sf,axis", [(11, 2, 2), (44, 3, 3), (15, 4, 3), (5, 1, 2)])
def test_resample_axis_with_guarded_tap_tables(n_in, sf, axis):
    """virnet_resample_axis reads its tap tables by index: the tables go through guard_input too (forward taps, then the transposed ones)."""
    idx, wgt = degrade.tap_table(n_in, sf)
    idx_t, wgt_t = degrade.transpose_taps(idx, wgt, n_in)
    shape = [2, 3, 7, 9]
    shape[axis] = n_in
    src = torch.rand(shape, generator=torch.Generator().manual_seed(7)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (idx, wgt, idx_t, wgt_t)]
    (down,), _ = run_guarded(lambda src, i, w: (degrade._resample(src, i, w, axis, i.shape[0]),), dict(src=src, i=dev[0], w=dev[1]))
    assert down.dtype == torch.float64
    run_guarded(lambda src, i, w: degrade._resample(src, i, w, axis, n_in), dict(src=down.clone(), i=dev[2], w=dev[3]))


# ---- whole forwards: every intermediate tensor, SFT vector and packed image between zones -------------------------------------------------
def _forward_case(kind, shape):
    cfg = dict(SMALL)
    if kind == "denoise":              # SMALL without the SISR-only keys; noise_avg off, since the denoiser refuses it next to noise_cond
        cfg = dict({k: v for k, v in SMALL.items() if k not in ("kernel_chn", "dep_K", "kernel_cond")}, noise_avg=False)
    x = synth_images(*shape, seed=5).cuda()

    def build():
        net = (VIRAttResUNet if kind == "denoise" else VIRAttResUNetSR)(**cfg)
        net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=5), strict=True)
        return net.cuda().eval()

    def forward(net, x):
        with torch.no_grad():
            return net(x) if kind == "denoise" else net(x, 2)
    plain = forward(build(), x)
    with guarded() as g:
        net = g.adopt(build())                                    # built inside the guard; its parameters move into arenas
        out = forward(net, g.input(x))
        g.check(out)
        assert len(g.arenas) > 50
    for a, b in zip(out, plain):
        assert same_bits(a, b)


@pytest.mark.parametrize("shape", [(2, 3, 17, 22), (1, 3, 9, 7)])
@pytest.mark.parametrize("kind", ["denoise", "sisr_x2"])
def test_whole_forward(kind, shape):
    _forward_case(kind, shape)
