"""Every T-emitting instantiation of the stride-1 3x3 convolution hosts (tests/t_emit_cases.py) on the device, through
ops.conv_mfma(emit=...).  Per row:
  (1) what ran is what the row records: the launch timer's name, virnet_conv_plan_query with the row's emit_rows on the descriptor of the
      call itself, virnet_conv_wx4_last_plan, and a TImage came back (a silent fall-back to re-laying fails);
  (2) the stored tensor against an fp64 convolution with the whole epilogue at 2e-5 (the bar of tests/test_conv_variants_gpu.py for the
      same arithmetic on the same make_conv / rnd data; bf16 rows on bf16-rounded operands), and bit for bit the NON-emitting call with the
      same grouping;
  (3) the T image against a HOST reference built from the stored tensor -- optional LeakyReLU as one fp32 multiply, hi = rne(v),
      lo = rne(v - hi) or one bf16 plane, placed by test_wgrad_f16_gpu.t_image_same -- over the whole buffer: t_acquire hands out zeros, so an
      element nobody wrote and a value written into a pad row / pad segment / x-pad both fail; and byte for byte virnet_chsplit of the
      stored tensor (which also covers the unused plane 1 of a bf16 image);
  (4) the channel sums, from partial workspaces that held NaN before the launch (a partial no wave writes poisons the sum), against the
      fp64 column sum of the stored tensor within 2e-5 * max(1, max |sum|) (tests/test_t_emit_gpu.py's bar); None where the row asks for none;
  (5) Winograd rows: the VIRNET_WX4_NREP=1 partner plans single slabs and gives the same stored bits and the same T bytes; its channel
      sums meet the same bar (the order of the partials differs).
A wrong T row or partial-sum offset in the second / third slab group (slab_base 3, 4, 5), in a single-slab emitting launch or with
cin != cout is silent everywhere else but in a slightly wrong weight gradient."""
import pytest
import torch

from t_emit_cases import ROWS, emit_mode, plain_env
from test_conv_variants_gpu import FAMILY, LAUNCH, TIMER_NAME, TOL, Case, planned, setenv
from test_ops_gpu import nchw
from test_t_emit_gpu import chsplit_ref
from test_wgrad_f16_gpu import t_image_same
from virnet_amd import ops

pytestmark = pytest.mark.gpu
EXTRA_KNOBS = ("VIRNET_WX4_EMIT_ROWS", "VIRNET_T_EMIT", "VIRNET_BIAS_FUSED", "VIRNET_WX4_MIN_SLAB_WGS")


class TCase(Case):
    """variant_cases' Case with an `emit` argument on its one call; run() -> (stored tensors, Launches record, timer names, TImages)"""
    emit = None

    def calls(self):
        [(stride, kw)] = super().calls()
        return [(stride, kw if self.emit is None else dict(kw, emit=self.emit))]

    def run(self):
        outs, rec, names = super().run()
        return [o for o in outs if not isinstance(o, ops.TImage)], rec, names, [o for o in outs if isinstance(o, ops.TImage)]


def env(monkeypatch, knobs):
    for k in EXTRA_KNOBS:
        monkeypatch.delenv(k, raising=False)
    setenv(monkeypatch, knobs)


def poison_partials(row, device):
    """NaN into both alternating partial-sum workspaces of ops.conv_mfma, at the size the row's launch asks for"""
    th, waves = (16, 8) if row.emit_rows == 16 else (8, 4)
    nblk = row.n * ((row.h + th - 1) // th) * ((row.w + 31) // 32) * waves
    for turn in (0, 1):
        buf = ops._workspace("emit_col%d" % turn, nblk * row.cout * 4, device)
        buf[:buf.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    return nblk


def emitting_run(case, row, launches):
    """one emitting call under the environment already set -> (stored tensor, TImage, channel sums | None); checks (1)"""
    nblk = poison_partials(row, case.dev["x"].device)
    case.emit = emit_mode(row)
    try:
        outs, rec, names, timgs = case.run()
    finally:
        case.emit = None
    assert names == [TIMER_NAME[row.family]], names
    assert len(rec.convs) == 1 and len(outs) == 1 and len(timgs) == 1, (len(rec.convs), len(outs), timgs)      # (no TImage: a silent fall-back to re-laying)
    d, form, te = rec.convs[0]
    assert te is not None and te.rows == (row.emit_rows if row.family == "wx4" else 0) and bool(te.bf16) == (row.family == "bf16")
    plan = [tuple(l[k] for k in LAUNCH) for l in ops.conv_plan_query(FAMILY[row.family], d, emit_rows=row.emit_rows)]
    assert plan == launches, (plan, launches)
    if row.family == "wx4":
        first = launches[0]
        assert ops.wx4_last_plan() == {"rows": first[1], "persistent": False, "slabs": first[3], "launches": len(launches)}
    timg = timgs[0]
    assert timg.buf is not None and timg.bf16 == (row.family == "bf16") and (timg.n, timg.h, timg.w, timg.c) == (row.n, row.h, row.w, row.cout)
    if emit_mode(row)["colsum"] is not None:
        assert timg.nblk == nblk and timg.ncol == row.cout
    sums = timg.bias_sums()                                # (now: the second-next emitting conv overwrites the partials)
    return outs[0], timg, sums


def check_sums(sums, y, row, what):
    if emit_mode(row)["colsum"] is None:
        assert sums is None, what
        return 0.0
    colsum = y.double().sum((0, 1, 2))
    err = float((sums.double() - colsum).abs().max())          # (NaN: a partial nobody wrote)
    bar = 2e-5 * max(1.0, float(colsum.abs().max()))
    assert tuple(sums.shape) == (row.cout,) and err <= bar, (what, err, bar)
    return err


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_emitting_variant_against_fp64_and_a_host_t_image(monkeypatch, row):
    ops.t_pool_clear()                                     # every T buffer of this test is a fresh, zeroed one
    case = TCase(row)
    [ref] = case.reference()
    bf16, tslope = row.family == "bf16", emit_mode(row)["act"]
    # (1) under the row's knobs
    env(monkeypatch, row.env)
    y, timg, sums = emitting_run(case, row, row.launches)
    # (2) the stored tensor: fp64, then the non-emitting call with the same grouping
    assert tuple(nchw(y).shape) == tuple(ref.shape)
    err = float((nchw(y).double() - ref).abs().max())
    env(monkeypatch, plain_env(row))
    [y0], rec0, names0, none = case.run()
    assert not none and names0 == [TIMER_NAME[row.family]]
    plans0 = planned(rec0, row.family)
    assert plans0 == [row.launches], (plans0, row.launches)
    same_store = torch.equal(y, y0)
    # (3) the T image: host reference over the whole buffer, then virnet_chsplit's bytes
    a = nchw(y)
    if tslope is not None:
        a = torch.where(a > 0, a, a * tslope)
    bad = [int((~same).sum()) for same in t_image_same(timg.buf, a, bf16)]
    ref_bytes = chsplit_ref(y, bf16, tslope)
    assert ref_bytes.numel() == timg.buf.numel()
    diff = int((ref_bytes != timg.buf).sum())
    # (4) the channel sums
    serr = check_sums(sums, y, row, "row")
    print(f"{row.id}: max error against fp64 {err:.3e}, channel sums {serr:.3e}, T elements off {bad}, T bytes off chsplit {diff}")
    assert err <= TOL, err
    assert same_store, float((y - y0).abs().max())
    assert not any(bad), f"T elements that differ from the host image, per plane: {bad}"
    assert diff == 0, f"{diff} of {ref_bytes.numel()} bytes differ from virnet_chsplit"
    # (5) the single-slab grouping: the same stored bits, the same T bytes
    if row.family == "wx4":
        env(monkeypatch, row.single)
        y1, timg1, sums1 = emitting_run(case, row, row.single_launches)
        assert torch.equal(y, y1), float((y - y1).abs().max())
        diff1 = int((timg1.buf != timg.buf).sum())
        assert diff1 == 0, f"{diff1} T bytes differ between the row and its single-slab partner"
        check_sums(sums1, y, row, "partner")
