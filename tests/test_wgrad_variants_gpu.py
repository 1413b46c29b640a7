"""Every instantiation and plan edge of the f16-pipe weight gradient (tests/wgrad_cases.py) on the device, through ops.conv_wgrad /
ops.convt_wgrad.  Per row:
  (a) the f16 path ran (the launch timer's key), and for bf16 rows its bf16 form (the result is NOT the unrounded gradient);
  (b) every workspace of the stream is filled with 0xFF bytes (fp32 NaN) before the call, after a throw-away call of the same shape has
      grown them: the partial-sum scratch, both T images and the column partials are documented as fully written, so a result that depends
      on a stale element -- a run without steps that leaves its scratch slice alone, say -- is NaN;
  (c) dw and db against fp64 on the CPU from the operands the kernel sees (the fp32 staging transform, bf16 rounding of both operands for
      the bf16 form -- their products are exact in fp32; db always from the unrounded dy), at 2e-5 of the largest reference element: the
      bar tests/test_wgrad_f16_gpu.py holds the same kernels to against fp32 autograd;
  (d) a second call gives the same dw bit for bit.  db is NOT held to that: its column partials meet through atomicAdd in
      colpart_reduce_kernel (up to 64 slices per channel block, in arrival order), so it is held to the tolerance twice instead.
test_reduction_with_pending_bias_partials runs the stride-1 rows that pin the reduction (every number of runs mod 4, seventeen runs, empty
runs, a 16-channel record) once more with dy handed over as a T image whose column partials are still pending: the call then ends in
wgrad_reduce_db_kernel -- the same reduction body with the bias gradient's blocks behind it -- and must give the SAME dw bits.
Stored-but-unused channels (records of 16 channels with 4 / 3 real ones) carry finite junk of order 1e3, not zeros.

Largest measured error / max|ref| per mode on an MI355X, all rows (the bar is 2e-5; fp32 accumulation order is what is left):
  stride-1 3x3      dw 2.4e-07 (bf16 rows 1.1e-07)   db 1.6e-07
  stride-2 3x3      dw 2.1e-07 (bf16 rows 1.2e-07)   db 1.8e-07
  2x2 transposed    dw 1.7e-07 (bf16 rows 1.1e-07)   db 1.7e-07
Held against a library with two deliberate mistakes -- runs without steps skip their scratch store; wgrad_reduce_s2_kernel drops the last
run of its tail -- the module fails the stride-1 empty-run row (NaN) on both reduction routes and every stride-2 / transposed row whose
number of runs is not a multiple of four, and passes the rest."""
import pytest
import torch
import torch.nn.functional as F

from test_backward_gpu import relerr
from test_ops_gpu import nhwc, rnd
from test_redzone_gpu import Launches
from wgrad_cases import BY_ID, CONVT, ROWS, S1, S2
from virnet_amd import _native as nat
from virnet_amd import ops

pytestmark = pytest.mark.gpu
TOL = 2e-5
SLOPE = 0.2


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


class Case:
    """The tensors of a row (built once), the call on them and its fp64 reference."""

    def __init__(self, row):
        self.row = row
        n, h, w = row.n, row.h, row.w
        xs, ys = {S1: ((h, w), (h, w)), S2: ((2 * h, 2 * w), (h, w)), CONVT: ((h, w), (2 * h, 2 * w))}[row.mode]
        self.x, self.dy = rnd(n, row.cx, *xs, seed=400), rnd(n, row.cy, *ys, seed=401)
        if row.cx > row.cin:                                # stored, not part of the convolution: must not reach dw
            self.x[:, row.cin:] = rnd(n, row.cx - row.cin, *xs, seed=402, lo=500.0, hi=2000.0)
        if row.cy > row.cout:
            self.dy[:, row.cout:] = rnd(n, row.cy - row.cout, *ys, seed=403, lo=-2000.0, hi=-500.0)
        self.mul, self.add = rnd(n, row.cx, seed=404, lo=0.3, hi=1.2), rnd(n, row.cx, seed=405)
        self.dev = dict(x=nhwc(self.x), dy=nhwc(self.dy), mul=self.mul.cuda(), add=self.add.cuda())

    def call(self):
        row, d = self.row, self.dev
        if row.mode == CONVT:
            assert row.bias_channels == row.cout
            return ops.convt_wgrad(d["x"], d["dy"], (row.cin, row.cout, 2, 2))
        kw = dict(in_slope=SLOPE) if row.pre >= 1 else {}
        if row.pre == 2:
            kw.update(in_mul=d["mul"], in_add=d["add"])
        return ops.conv_wgrad(d["x"], d["dy"], (row.cout, row.cin, 3, 3), stride=2 if row.mode == S2 else 1, bias_channels=row.bias_channels, **kw)

    def staged(self):
        """the forward conv's input as virnet_chsplit stages it, in fp32: one fused multiply-add (exact product, one rounding), then the
        LeakyReLU -- tests/test_wgrad_f16_gpu.py::test_chsplit_layout_is_exact holds the kernel to exactly this"""
        row, a = self.row, self.x
        if row.pre == 2:
            a = (a.double() * self.mul.double().view(row.n, row.cx, 1, 1) + self.add.double().view(row.n, row.cx, 1, 1)).float()
        if row.pre >= 1:
            a = F.leaky_relu(a, SLOPE)
        return a[:, :row.cin]

    def reference(self, rounded):
        """(dw, db) in fp64; rounded: both operands of the contraction rounded to bf16 first"""
        row = self.row
        a, g = self.staged(), self.dy[:, :row.cout]
        if rounded:
            a, g = bf16_round(a), bf16_round(g)
        a, g = a.double(), g.double()
        if row.mode == CONVT:
            wt = torch.zeros(row.cin, row.cout, 2, 2, dtype=torch.float64, requires_grad=True)
            F.conv_transpose2d(a, wt, None, stride=2).backward(g)
        else:
            wt = torch.zeros(row.cout, row.cin, 3, 3, dtype=torch.float64, requires_grad=True)
            F.conv2d(a, wt, None, stride=2 if row.mode == S2 else 1, padding=1).backward(g)
        return wt.grad, self.dy[:, :row.bias_channels].double().sum((0, 2, 3))


def poison_workspaces():
    """0xFF into every workspace buffer of the current stream: each fp32 (and each fp16 / bf16 pair) becomes a NaN"""
    dev = torch.cuda.current_device()
    stream = torch.cuda.current_stream().cuda_stream
    mine = [buf for (d, s, _), buf in ops._WORKSPACES.items() if d == dev and s == stream]
    for buf in mine:
        buf.fill_(0xFF)
    return len(mine)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_wgrad_variant_against_fp64_with_poisoned_scratch(monkeypatch, row):
    for k in ("VIRNET_WGRAD_FORM", "VIRNET_WINOGRAD"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VIRNET_CONV_FORM", "bf16" if row.bf16 else "f16x3")
    case = Case(row)
    dw_ref, db_ref = case.reference(bool(row.bf16))
    case.call()                                            # throw-away: grows the workspaces to this shape
    results = []
    for _ in range(2):
        assert poison_workspaces() >= 4                    # wgrad_xt, wgrad_yt, wgrad_col, wgrad_part
        with Launches() as rec:
            dw, db = case.call()
            assert rec.names() == ["wgrad_f16" if row.mode == S1 else "wgrad_f16_s2"], rec.names()
        results.append((dw.cpu().double(), db.cpu().double()))
    (dw, db), (dw2, db2) = results
    assert tuple(dw.shape) == tuple(dw_ref.shape) and tuple(db.shape) == (row.bias_channels,)
    e_dw, e_db, e_db2 = relerr(dw, dw_ref), relerr(db, db_ref), relerr(db2, db_ref)
    print(f"{row.id}: dw {e_dw:.3e} db {e_db:.3e} / {e_db2:.3e} of max|ref| {float(dw_ref.abs().max()):.3g} / {float(db_ref.abs().max()):.3g}")
    assert e_dw <= TOL, e_dw                               # (a NaN fails every comparison)
    assert e_db <= TOL and e_db2 <= TOL, (e_db, e_db2)     # atomicAdd order: tolerance, not bits
    assert torch.equal(dw, dw2)                            # fixed-order reduction, no atomics
    if row.bf16:
        # the bf16 form ran: against the UNROUNDED operands the error is that of 2^-9 roundings, far above the bar
        assert relerr(dw, case.reference(False)[0]) > 10 * TOL


DB_ROUTE = ["kg4nwv1-s1-bf16-c32to32-n2h8w66", "kg4nwv1-s1-f16-c32to32-n2h5w65", "kg4nwv2-s1-f16-c32to64-n2h6w65", "kg4nwv3-s1-f16-c32to96-n2h7w65",
            "runs17-s1-f16-c32to32-n2h17w65", "empty2-s1-f16-c224to288-n2h25w64", "record-s1-f16-c96to3-n2h8w33"]


@pytest.mark.parametrize("rid", DB_ROUTE)
def test_reduction_with_pending_bias_partials(monkeypatch, rid):
    row = BY_ID[rid]
    for k in ("VIRNET_WGRAD_FORM", "VIRNET_WINOGRAD"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VIRNET_CONV_FORM", "bf16" if row.bf16 else "f16x3")
    case = Case(row)
    dw_ref, db_ref = case.reference(bool(row.bf16))
    dw_plain, _ = case.call()                              # (also grows the workspaces)
    # the T image of dy with its per-block channel sums left unreduced, as an emitting convolution hands it over (virnet_chsplit writes
    # the partials only on its way to a db, so it gets a throw-away one)
    lib, n, h, w, cy = nat.load(), row.n, row.h, row.w, row.cy
    buf = torch.full((lib.virnet_chsplit_bytes(n, h, w, cy),), 0xFF, dtype=torch.uint8, device="cuda")
    col = torch.full((lib.virnet_chsplit_colsum_bytes(n, h, w, cy) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    scrap = torch.zeros(row.bias_channels, dtype=torch.float32, device="cuda")
    nat.check(lib.virnet_chsplit(nat.ptr(case.dev["dy"]), n, h, w, cy, 0, 0.0, None, None, row.bf16, nat.ptr(buf), nat.ptr(col), nat.ptr(scrap),
                                 row.bias_channels, nat.stream_handle()), "chsplit")
    nseg = 6 if w <= 32 else 8 * ((w + 63) // 64) + 2
    yt = ops.TImage(buf=buf, n=n, h=h, w=w, c=cy, bf16=bool(row.bf16), col=col, nblk=n * (h + 2) * ((nseg + 7) // 8), ncol=row.bias_channels)
    assert poison_workspaces() >= 4
    kw = dict(in_slope=SLOPE) if row.pre >= 1 else {}
    if row.pre == 2:
        kw.update(in_mul=case.dev["mul"], in_add=case.dev["add"])
    with Launches() as rec:
        dw, db = ops.conv_wgrad(case.dev["x"], case.dev["dy"], (row.cout, row.cin, 3, 3), bias_channels=row.bias_channels, yt=yt, **kw)
        assert rec.names() == ["wgrad_f16"], rec.names()
    assert yt.col is None and yt.db is db                  # the partials were consumed by THIS call's reduction launch
    e_dw, e_db = relerr(dw.cpu().double(), dw_ref), relerr(db.cpu().double(), db_ref)
    print(f"{row.id} (db route): dw {e_dw:.3e} db {e_db:.3e}")
    assert e_dw <= TOL and e_db <= TOL, (e_dw, e_db)
    assert torch.equal(dw, dw_plain)
