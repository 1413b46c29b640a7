"""tests/small_cases.py against the host launch code of csrc/small.hip (and the two branches ops.py adds), without a device.

1. The host branches are written out below as data, each with the source line it comes from; the line must still hold the quoted text.
2. `branches(row)` restates the launch arithmetic in Python (the ppb doubling, grid caps, vv, kSftChunk, the 256-thread loops) next to a
   pointer to the C line, and the table must reach every listed branch -- and no row may claim one the list does not know.
3. The table spans the value sets it is there for (image sizes mod 4, ow, n*oh mod 4, channel counts, hw on both sides of each limit ...).
4. The table is exactly the rows listed: deleting one fails here.
5. For every row whose kernel reduces over pixels (gap, the CALayer mean, the head's weight gradient, dmul / dadd) the fp64 reference is
   computed twice, in full and with ONE term removed from each sum, and the two must differ by more than 4 x the row's bar: a bar that a
   dropped term would pass is a test that cannot fail.
6. The sft_backward rows keep |x*mul+add| >= 1e-3 in fp64 everywhere (but at the exact zeros of the zero row): no element is excluded."""
import os

import pytest
import torch

import small_cases as sc
from small_cases import BY_ID, ROWS, out_hw

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP, OPS = "virnet_amd/csrc/small.hip", "virnet_amd/ops.py"

# branch -> (file, line, text that line holds)
BRANCHES = {
    "head.ppb=4": (HIP, 495, "while ((npix + ppb - 1) / ppb > 4096) ppb *= 2;"),
    "head.ppb=8": (HIP, 495, "while ((npix + ppb - 1) / ppb > 4096) ppb *= 2;"),
    "head.ctiles=1": (HIP, 497, "dim3(gx, cout / 64)"),
    "head.ctiles=2": (HIP, 497, "dim3(gx, cout / 64)"),
    "head.refuse_lds": (HIP, 482, "lds <= 160 * 1024"),
    "wgrad.tail": (HIP, 93, "if (ox < ow) {"),
    "wgrad.notail": (HIP, 93, "if (ox < ow) {"),
    "wgrad.co0=1": (HIP, 77, "for (int co0 = 0; co0 < cout; co0 += 64)"),
    "wgrad.co0=2": (HIP, 77, "for (int co0 = 0; co0 < cout; co0 += 64)"),
    "dgrad.onepass": (HIP, 519, "(total + 255) / 256 > 4096 ? 4096"),
    "dgrad.gridstride": (HIP, 519, "(total + 255) / 256 > 4096 ? 4096"),
    "scale_add.onepass": (HIP, 550, "(total4 + 255) / 256 > 8192 ? 8192"),
    "scale_add.gridstride": (HIP, 550, "(total4 + 255) / 256 > 8192 ? 8192"),
    "ca.refuse_c": (HIP, 538, "256 % c == 0"),
    "fused.V=4": (HIP, 570, "if (vv <= 4)"),
    "fused.V=8": (HIP, 571, "else if (vv <= 8)"),
    "fused.V=16": (HIP, 572, "ca_scale_add_kernel<16>"),
    "fused.refuse_items": (HIP, 564, "n4 <= 16 * 1024"),
    "fused.fallback": (OPS, 996, "h * w * (c // 4) > CA_FUSED_MAX_ITEMS"),
    "sftb.chunks=1": (HIP, 589, "constexpr int kSftChunk = 1024;"),
    "sftb.chunks=2": (HIP, 589, "constexpr int kSftChunk = 1024;"),
    "sftb.chunks=3": (HIP, 589, "constexpr int kSftChunk = 1024;"),
    "sftb.pl_n=1": (HIP, 294, "const int pl_n = 256 / c4;"),
    "sftb.c4_not_dividing_256": (HIP, 297, "if (pl < pl_n) {"),
    "sft_vec.chanloop=1": (HIP, 372, "for (int c = threadIdx.x; c < wt.nf; c += 256)"),
    "sft_vec.chanloop=2": (HIP, 372, "for (int c = threadIdx.x; c < wt.nf; c += 256)"),
    "sft_apply.chanloop=1": (HIP, 443, "for (int c = threadIdx.x; c < wt.nf; c += 256)"),
    "sft_apply.chanloop=2": (HIP, 443, "for (int c = threadIdx.x; c < wt.nf; c += 256)"),
    "sft.refuse_widths": (HIP, 468, "wt->nf1 <= 64"),
    "sft_apply.refuse_record": (HIP, 655, "chan0 + wt->e <= 16"),
    "sft_multi.launches=1": (OPS, 1080, "for i0 in range(0, len(atts), SFT_MULTI_MAX):"),
    "sft_multi.launches=2": (OPS, 1080, "for i0 in range(0, len(atts), SFT_MULTI_MAX):"),
    "sft_multi.launches=3": (OPS, 1080, "for i0 in range(0, len(atts), SFT_MULTI_MAX):"),
    "gap.hw<256": (HIP, 159, "for (int i = threadIdx.x; i < hw; i += 256) s += p[i];"),
    "gap.hw=256": (HIP, 159, "for (int i = threadIdx.x; i < hw; i += 256) s += p[i];"),
    "gap.hw>256": (HIP, 159, "for (int i = threadIdx.x; i < hw; i += 256) s += p[i];"),
    "poison.onepass": (HIP, 676, "(n + 255) / 256 > 1024 ? 1024"),
    "poison.gridstride": (HIP, 676, "(n + 255) / 256 > 1024 ? 1024"),
}


def cdiv(a, b):
    return -(-a // b)


def head_ppb(npix):
    """virnet_conv_head_s4, small.hip:494-495"""
    ppb = 4
    while cdiv(npix, ppb) > 4096:
        ppb *= 2
    return ppb


def fused_v(n4):
    """virnet_ca_scale_add, small.hip:565-572: vv = ceil(n4 / 1024) -> the instantiation; None past the 16 * 1024 limit (small.hip:564)"""
    if n4 > 16 * 1024:
        return None
    vv = cdiv(n4, 1024)
    return 4 if vv <= 4 else 8 if vv <= 8 else 16


def branches(row):
    """the host branches the row's launch takes, from its shape alone"""
    s, f, refuse = row.shape, row.family, row.opt.get("refuse")
    if f == "head":
        if s["cin"] * 81 * (65 + 4) * 4 > 160 * 1024:                             # small.hip:481-482, K * 65 + 4 * K floats
            return {"head.refuse_lds"}
        oh, ow = out_hw(s["h"], s["w"])
        return {f"head.ppb={head_ppb(s['n'] * oh * ow)}", f"head.ctiles={s['cout'] // 64}"}
    if f == "head_wgrad":
        ow = out_hw(s["h"], s["w"])[1]
        return {"wgrad.tail" if ow % 2 else "wgrad.notail", f"wgrad.co0={cdiv(s['cout'], 64)}"}   # small.hip:88-93 (ox + 1 < ow pairs), :77
    if f == "head_dgrad":
        total = s["n"] * s["cin"] * s["h"] * s["w"]
        return {"dgrad.gridstride" if cdiv(total, 256) > 4096 else "dgrad.onepass"}               # small.hip:518-519
    if f == "gap":
        hw = s["h"] * s["w"]
        return {"gap.hw<256" if hw < 256 else "gap.hw=256" if hw == 256 else "gap.hw>256"}
    if f in ("ca", "scale_add"):
        if f == "ca" and 256 % s["c"]:
            return {"ca.refuse_c"}
        total4 = s["n"] * s["h"] * s["w"] * (s["c"] // 4)
        return {"scale_add.gridstride" if cdiv(total4, 256) > 8192 else "scale_add.onepass"}      # small.hip:549-550
    if f == "fused":
        v = fused_v(s["h"] * s["w"] * (s["c"] // 4))
        if v is None:
            return {"fused.fallback"} if row.opt.get("fallback") else {"fused.refuse_items"}
        return {f"fused.V={v}"}
    if f == "sft_backward":
        c4 = s["c"] // 4
        out = {f"sftb.chunks={cdiv(s['hw'], 1024)}"}                                # small.hip:581 / :607, chunk = kSftChunk = 1024
        if 256 // c4 == 1:
            out.add("sftb.pl_n=1")
        if 256 % c4:
            out.add("sftb.c4_not_dividing_256")
        return out
    if f in ("sft_vec", "sft_apply"):
        if s["nf"] // 8 > 64 or s["nf"] // 4 > 128 or s["e"] > 16:               # AttLayer: nf1 = nf // 8, nf2 = nf // 4
            return {"sft.refuse_widths"}
        if f == "sft_apply" and s["chan0"] + s["e"] > 16:
            return {"sft_apply.refuse_record"}
        return {f"{f}.chanloop={cdiv(s['nf'], 256)}"}
    if f == "sft_multi":
        return {f"sft_multi.launches={cdiv(s['layers'], 16)}"}                      # ops.py:1080, SFT_MULTI_MAX = 16
    if f == "poison":
        return {"poison.gridstride" if cdiv(s["n"], 256) > 1024 else "poison.onepass"}
    raise KeyError(f)


IDS = """
head-n1c1h1w1-o64 head-n1c3h3w4-o64 head-n3c3h4w5-o64 head-n3c3h4w5-o128 head-n2c3h21w30-o64 head-n2c3h21w30-o128 head-n1c4h9w7-o64
head-n5c3h5w8-o64 head-n3c2h2w2-o64 head-n2c7h6w9-o128 head-n1c1h516w516-o64 head-n1c8h4w4-o64
hwgrad-n1c1h3w4-o64 hwgrad-n3c3h4w5-o96 hwgrad-n1c3h8w18-o128 hwgrad-n2c3h21w30-o64 hwgrad-n5c1h5w8-o64 hwgrad-n1c3h592w592-o64
hdgrad-n1c3h64w64-o64 hdgrad-n3c3h57w86-o64 hdgrad-n1c3h9w7-o64 hdgrad-n3c3h13w13-o64 hdgrad-n1c3h9w7-o4 hdgrad-n3c3h13w13-o96
hdgrad-n1c3h592w592-o64
gap-n3c3h1w1-mean gap-n3c3h1w1-kinfo gap-n2c3h7w9-expclamp gap-n3c1h15w17-kinfo gap-n2c3h16w16-mean gap-n2c3h16w16-expclamp
gap-n3c3h1w257-kinfo gap-n1c3h481w321-mean
ca-n2h1w1-c4r1 ca-n2h1w3-c64r4 ca-n2h1w3-c4r64 ca-n2h15w17-c64r4 ca-n1h257w1-c256r64 ca-n1h3w85-c256r1 ca-n3h1w257-c4r4 ca-n1h1w1-c96r4
scaleadd-n1h363w363-c64
fused-n3hw1-c4r1 fused-n3hw4096-c4r1 fused-n3hw4097-c4r1 fused-n3hw8192-c4r4 fused-n3hw8193-c4r4 fused-n3hw16384-c4r4 fused-n3hw256-c64r4
fused-n3hw257-c64r4 fused-n3hw512-c64r4 fused-n3hw513-c64r4 fused-n3hw1024-c64r4 fused-n3hw64-c256r64 fused-n3hw16385-c4r1
fallback-n3hw16385-c4r1
sftvec-nf96e4 sftvec-nf288e4 sftvec-nf512e16 sftvec-nf64e1 sftvec-nf520e4
sftmulti-l1 sftmulti-l16 sftmulti-l17 sftmulti-l33
sftapply-nf96e4-n1h3w5-s1k0 sftapply-nf288e4-n2h2w4-s2k3 sftapply-nf512e16-n1h1w17-s4k0 sftapply-nf64e1-n3h5w1-s2k3
sftapply-nf104e13-n1h17w1-s1k3 sftapply-nf104e13-n1h4w4-s1k4
sftb-n1hw1c4-nores sftb-n3hw1c1024-nores sftb-n3hw1023c8-res sftb-n1hw1024c96-res sftb-n3hw1025c96-nores sftb-n1hw2049c1024-res
sftb-n3hw2049c4-nores sftb-n1hw33c8-res-zero
poison-n1 poison-n255 poison-n262145
""".split()


def vals(family, fn, refused=False):
    return {fn(r.shape) for r in sc.rows(family, refused)}


def test_branch_list_points_at_the_lines_it_quotes():
    text = {}
    for name, (path, line, quote) in BRANCHES.items():
        if path not in text:
            with open(os.path.join(REPO, path)) as f:
                text[path] = f.read().split("\n")
        assert quote in text[path][line - 1], f"{name}: {path}:{line} is now {text[path][line - 1].strip()!r}"


def test_table_reaches_every_listed_branch_and_no_other():
    got = set().union(*(branches(r) for r in ROWS))
    assert not set(BRANCHES) - got, sorted(set(BRANCHES) - got)
    assert not got - set(BRANCHES), sorted(got - set(BRANCHES))            # a branch the list above does not know: extend it


def test_refusal_rows_are_exactly_the_rows_whose_branch_is_a_refusal():
    for r in ROWS:
        refusal = any(".refuse" in b for b in branches(r))
        assert refusal == bool(r.opt.get("refuse")), r.id


def test_table_is_exactly_the_listed_rows():
    assert len(set(IDS)) == len(IDS) == len(ROWS)
    assert [r.id for r in ROWS] == IDS
    assert len(BY_ID) == len(ROWS)
    for r in ROWS:
        assert r.why and all(e.startswith("virnet_") for e in r.entries), r.id


def test_every_entry_of_the_table_is_bound_and_every_small_entry_has_a_row():
    from virnet_amd import _native
    bound = {name for name, _, _ in _native.SYMBOLS}
    used = {e for r in ROWS for e in r.entries}
    assert used <= bound, used - bound
    with open(os.path.join(REPO, HIP)) as f:
        src = f.read()
    exported = {name for name in bound if f'extern "C" int {name}(' in src}
    assert exported == used, exported ^ used                                # the thirteen launching entries of small.hip


def test_head_forward_rows_span_their_sets():
    npix = [s["n"] * out_hw(s["h"], s["w"])[0] * out_hw(s["h"], s["w"])[1] for s in (r.shape for r in sc.rows("head"))]
    assert {p % 4 for p in npix} == {0, 1, 2, 3}
    assert vals("head", lambda s: s["h"] % 4) == {0, 1, 2, 3} and vals("head", lambda s: s["w"] % 4) == {0, 1, 2, 3}
    listed = {(1, 1, 1, 1), (1, 3, 3, 4), (3, 3, 4, 5), (2, 3, 21, 30), (1, 4, 9, 7), (5, 3, 5, 8), (1, 1, 516, 516)}
    assert listed <= vals("head", lambda s: (s["n"], s["cin"], s["h"], s["w"]))
    assert vals("head", lambda s: s["cout"]) == {64, 128} and max(vals("head", lambda s: s["cin"])) == 7
    assert vals("head", lambda s: s["cin"], refused=True) == {8}
    big = BY_ID["head-n1c1h516w516-o64"]
    assert 129 * 129 == 16641 and head_ppb(16641) == 8 and head_ppb(16384) == 4 and big.opt["crop"] == 64
    assert head_ppb(out_hw(64, 64)[0] * out_hw(64, 64)[1]) == 4            # the crop run
    assert 7 * 81 * 69 * 4 == 156492 <= 160 * 1024 < 8 * 81 * 69 * 4


def test_head_gradient_rows_span_their_sets():
    assert vals("head_wgrad", lambda s: out_hw(s["h"], s["w"])[1]) >= {1, 2, 5, 8}
    assert vals("head_wgrad", lambda s: s["n"] * out_hw(s["h"], s["w"])[0] % 4) == {0, 1, 2, 3}
    assert vals("head_wgrad", lambda s: s["cout"]) == {64, 96, 128} and vals("head_wgrad", lambda s: s["cin"]) == {1, 3}
    assert [r.id for r in sc.rows("head_wgrad") if r.opt.get("long")] == ["hwgrad-n1c3h592w592-o64"]
    assert {(1, 64, 64), (3, 57, 86), (1, 9, 7), (3, 13, 13)} <= vals("head_dgrad", lambda s: (s["n"], s["h"], s["w"]))
    assert vals("head_dgrad", lambda s: s["cout"]) == {4, 64, 96}
    assert 3 * 592 * 592 == 1051392 > 4096 * 256


def test_gap_rows_span_their_sets():
    assert vals("gap", lambda s: s["h"] * s["w"]) == {1, 63, 255, 256, 257, 481 * 321}
    assert {r.opt["finish"] for r in sc.rows("gap")} == {sc.GAP_MEAN, sc.GAP_EXPCLAMP, sc.GAP_KINFO}
    assert {r.shape["c"] for r in sc.rows("gap") if r.opt["finish"] == sc.GAP_KINFO} == {1, 3}
    lo, hi = sc.CLAMP
    for r in sc.rows("gap"):
        if r.opt["finish"] == sc.GAP_MEAN or r.shape["c"] == 1:
            continue
        m = sc.case(r.id).inp["x"].double().mean((2, 3))
        m = m[:, :r.shape["c"] - 1] if r.opt["finish"] == sc.GAP_KINFO else m     # the channels that go through exp(clamp)
        assert bool((m < lo).any()) and bool(((m > lo) & (m < hi)).any()) and bool((m > hi).any()), r.id


def test_calayer_rows_span_their_sets():
    assert vals("ca", lambda s: s["c"]) == {4, 64, 256} and vals("ca", lambda s: s["cr"]) == {1, 4, 64}
    assert vals("ca", lambda s: s["h"] * s["w"]) == {1, 3, 255, 257}
    assert any(s["h"] * s["w"] < 256 // s["c"] for s in (r.shape for r in sc.rows("ca")))      # fewer pixels than pixel phases
    assert vals("ca", lambda s: s["c"], refused=True) == {96}
    s = BY_ID["scaleadd-n1h363w363-c64"].shape
    assert s["n"] * s["h"] * s["w"] * s["c"] // 4 == 2108304 > 8192 * 256
    fused = sc.rows("fused")
    assert all(r.shape["n"] == 3 for r in fused + sc.rows("fused", True))
    assert {r.shape["w"] for r in fused if r.shape["c"] == 4 and not r.opt.get("fallback")} == {1, 4096, 4097, 8192, 8193, 16384}
    assert {r.shape["w"] for r in fused if r.shape["c"] == 64} == {256, 257, 512, 513, 1024}
    assert {(r.shape["w"], r.shape["cr"]) for r in fused if r.shape["c"] == 256} == {(64, 64)}
    for hw, c, v in ((4096, 4, 4), (4097, 4, 8), (8192, 4, 8), (8193, 4, 16), (16384, 4, 16), (256, 64, 4), (257, 64, 8), (512, 64, 8), (513, 64, 16)):
        assert fused_v(hw * c // 4) == v
    over = [r for r in ROWS if r.family == "fused" and r.shape["w"] * r.shape["c"] // 4 == 16385]
    assert sorted(bool(r.opt.get("refuse")) for r in over) == [False, True] and fused_v(16385) is None


def test_sft_rows_span_their_sets():
    assert vals("sft_vec", lambda s: (s["nf"], s["e"])) == {(96, 4), (288, 4), (512, 16), (64, 1)}
    assert (512 // 8, 512 // 4) == (64, 128) and 520 // 8 == 65
    assert vals("sft_vec", lambda s: (s["nf"], s["e"]), refused=True) == {(520, 4)}
    assert vals("sft_multi", lambda s: s["layers"]) == {1, 16, 17, 33}
    ap = sc.rows("sft_apply")
    assert {s["n"] * s["h"] * s["w"] for s in (r.shape for r in ap)} == {15, 16, 17}
    assert {r.shape["step"] for r in ap} == {1, 2, 4} and {r.shape["chan0"] for r in ap} == {0, 3}
    assert any(r.shape["e"] == 13 and r.shape["chan0"] == 3 for r in ap)
    assert vals("sft_apply", lambda s: s["chan0"] + s["e"], refused=True) == {17}
    sb = sc.rows("sft_backward")
    assert {r.shape["c"] for r in sb} == {4, 8, 96, 1024} and {r.shape["n"] for r in sb} == {1, 3}
    assert {r.shape["hw"] for r in sb if not r.opt.get("zero")} == {1, 1023, 1024, 1025, 2049}
    assert {r.opt["res"] for r in sb} == {True, False} and sum(bool(r.opt.get("zero")) for r in sb) == 1
    assert {r.id for r in sb if r.opt.get("long")} == {r.id for r in sb if r.shape["hw"] == 2049}
    assert vals("poison", lambda s: s["n"]) == {1, 255, 256 * 1024 + 1}


@pytest.mark.parametrize("rid", [r.id for r in sc.rows("sft_backward")])
def test_sft_backward_rows_stay_off_the_kink(rid):
    inp = sc.case(rid).inp
    u = (inp["x"].double() * inp["mul"].double()[:, None, :] + inp["add"].double()[:, None, :]).abs()
    zero = inp.get("zero")
    if zero is None:
        assert float(u.min()) >= sc.KINK
    else:
        assert int(zero.sum()) == 22 and bool((u[zero] == 0).all()) and float(u[~zero].min()) >= sc.KINK
        ref = sc.case(rid).ref                                 # at u == 0: dx - res = slope * da * mul
        want = (sc.SLOPE * inp["da"].double() * inp["mul"].double()[:, None, :] + inp["res"].double())[zero]
        assert torch.equal(ref["dx"][zero], want)
        x0, m0, a0 = (inp[k].clone().requires_grad_(True) for k in ("x", "mul", "add"))      # ... which is what torch's backward gives
        torch.nn.functional.leaky_relu(x0 * m0[:, None, :] + a0[:, None, :], sc.SLOPE).backward(inp["da"])
        assert float((x0.grad.double() + inp["res"].double() - ref["dx"])[zero].abs().max()) <= 1e-7


REDUCTION_ROWS = [r.id for r in ROWS if r.family in sc.REDUCED and not r.opt.get("refuse")]


@pytest.mark.parametrize("rid", REDUCTION_ROWS)
def test_a_dropped_term_is_four_bars_away(rid):
    c = sc.case(rid)
    short = sc.reference(c.row, c.inp, drop=True)
    for key in sc.REDUCED[c.row.family]:
        d, b = float((short[key] - c.ref[key]).abs().max()), c.bar(key)
        print(f"{rid} {key}: a dropped term moves the reference by {d:.3e}, bar {b:.3e}" + (f", E32 {c.e32[key]:.3e}" if c.e32 else ""))
        assert d > 4 * b, (key, d, b)
    if c.e32:                                                  # the long rows: the existing bar or 4 x E32, whichever is larger
        for key, e in c.e32.items():
            assert c.bar(key) == max(sc.EXISTING_BAR[(c.row.family, key)] * max(1.0, float(c.ref[key].abs().max())), 4 * e)
