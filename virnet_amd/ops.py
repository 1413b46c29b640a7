"""Tensor-level wrappers over the C ABI: torch supplies device memory and the stream, nothing else.

Activations between kernels are NHWC fp32 tensors ``[N, H, W, C]`` (C a multiple of 16); images and the
returned maps are NCHW like the reference's.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _native as nat

Tensor = torch.Tensor


@dataclass
class PackedWeight:
    """MFMA-stage image of one conv / transposed-conv weight plus the plan it was packed for."""
    w: Tensor            # flat fp32 device tensor
    bias: Optional[Tensor]
    ks: int              # GEMM taps per side (1 for the transposed conv)
    cout: int
    cin_real: int
    cin_pad: int
    n_pad: int
    nrep: int
    transposed: bool
    wino: Optional[Tensor] = None   # Winograd-domain image (virnet_pack_wino_weight) of a stride-1 3x3 layer, when eligible
    f16: Optional[Tensor] = None    # split-fp16 image (virnet_pack_f16_weight) of a stride-1 3x3 layer, when eligible
    bf16: Optional[Tensor] = None   # bf16-operand image (virnet_pack_bf16_weight) of a C->C stride-1 3x3 layer (form "bf16" only)
    wx4: Optional[Tensor] = None    # Winograd F(4,3)-along-x split-fp16 image (virnet_pack_wx4_weight) of a C->C stride-1 3x3 layer (form "wx4")
    exit: Optional[Tensor] = None   # taps-as-rows split-fp16 image (virnet_pack_exit_weight) of a 3x3 layer with <= 3 output channels
    entry: Optional[Tensor] = None  # kernel-row-per-k-step split-fp16 image (virnet_pack_entry_weight) of a 3x3 layer with <= 8 input channels (csrc/conv_entry.hip)
    s2: Optional["PackedWeight"] = None   # dgrad packing of the 2x2 transposed conv: the same GEMM as a 3x3 stride-2 conv (convt_dgrad)


class LaunchTimer:
    """Optional per-launch HIP-event timing of the MFMA convolutions (used by bench.py for the roofline line).

    Events are recorded on torch's current stream, which is the stream the kernels are launched on."""

    def __init__(self):
        self.records = []   # (variant tuple, algorithmic flops, start event, end event)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for var, flops, e0, e1 in self.records:
            d = out.setdefault(var, {"launches": 0, "ms": 0.0, "flops": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
        return out


_TIMER: Optional[LaunchTimer] = None


def set_launch_timer(t: Optional[LaunchTimer]) -> None:
    global _TIMER
    _TIMER = t


def _timer_start():
    """Start of a timed span of several launches (the weight gradients and their re-layout passes): the span's two events, the first
    one recorded -- or None when no timer is set.  The only place that creates timing events."""
    if _TIMER is None:
        return None
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    return ev


def _timer_stop(ev, key: tuple, flops: float) -> None:
    ev[1].record()
    _TIMER.records.append((key, flops) + ev)


def _timed_call(fn, args: tuple, what: str, key, flops: float) -> None:
    """``fn(*args, stream)`` -- every single-launch entry point of the library goes through here -- and, when a timer is set, its record
    ``(key, flops, start, end)``.  ``key``: the tuple bench.py reads, or a callable that builds it (evaluated only under a timer)."""
    if _TIMER is None:
        nat.check(fn(*args, nat.stream_handle()), what)
        return
    if callable(key):
        key = key()
    ev = _timer_start()
    nat.check(fn(*args, nat.stream_handle()), what)
    _timer_stop(ev, key, flops)


# form -> (the library's entry point, the PackedWeight image it reads, its name in error messages)
_CONV_FORMS = {"direct": ("virnet_conv_mfma", "w", "conv_mfma"), "wino": ("virnet_conv_wino", "wino", "conv_wino"),
               "f16x3": ("virnet_conv_f16", "f16", "conv_f16"), "bf16": ("virnet_conv_bf16", "bf16", "conv_bf16"),
               "wx4": ("virnet_conv_wx4", "wx4", "conv_wx4"), "wx4x1": ("virnet_conv_wx4x1", "wx4", "conv_wx4x1")}


def _conv_key(d: "nat.ConvDesc", form: str, what: str) -> tuple:
    if form != "direct":
        return (form + ("_s2" if d.stride == 2 else "_t" if d.epi == nat.EPI_CONVT else ""), d.cout)
    var = (C.c_int * 4)()
    nat.check(nat.load().virnet_conv_mfma_variant(C.byref(d), C.byref(var)), what)
    return tuple(var)


def _launch_conv(d: "nat.ConvDesc", flops: float, what: str, form: str = "direct", te: Optional["nat.TEmit"] = None) -> None:
    lib = nat.load()
    if te is None:
        fn, args = getattr(lib, _CONV_FORMS[form][0]), (C.byref(d),)
    elif form == "wx4":                                  # the same launch + T emission (csrc: TE = 1 instantiations)
        fn, args = lib.virnet_conv_wx4_emit, (C.byref(d), C.byref(te))
    else:
        fn, args = lib.virnet_conv_f16_emit, (C.byref(d), C.byref(te), int(form == "bf16"))
    _timed_call(fn, args, what, lambda: _conv_key(d, form, what), flops)


# Forms of the stride-1 3x3 convolution whose channel counts fill MFMA blocks (read per call: tests flip it):
#   VIRNET_CONV_FORM=wx4     Winograd F(4,3) along x on the f16 matrix pipe with split-fp16 position products (csrc/conv_f16_wx4.hip):
#                            half of f16x3's MFMAs; layers / shapes it does not cover run as f16x3.  =wx4x1: REDUCED precision, INFERENCE only -- the launches wx4 sends to the Winograd form with ONE fp16 product per position product (csrc/conv_f16_wx4x1.hip), every other launch as under wx4
#   VIRNET_CONV_FORM=f16x3   split-fp16 operands on the f16 matrix pipe (csrc/conv_f16.hip)
#   VIRNET_CONV_FORM=wino    Winograd F(2x2,3x3) on the fp32 matrix pipe (csrc/wino_row.hip)
#   VIRNET_CONV_FORM=direct  fp32 implicit GEMM (csrc/conv_mfma.hip)
#   VIRNET_CONV_FORM=bf16    REDUCED precision (BASELINE configs[4]'s training variant): the C->C stride-1 3x3 convs and their input-gradient
#                            GEMMs with bf16-rounded operands, one product per MAC; every other layer as f16x3
# (older spelling, honoured when VIRNET_CONV_FORM is unset: VIRNET_WINOGRAD=0 -> direct, VIRNET_WINOGRAD=1 -> wino)
WINO_MIN_CHANNELS = 32
DEFAULT_CONV_FORM = "wx4"


# ---- per-forward snapshot of the environment knobs and the stream handle.  A single-image forward is ~45-100 launches and is bound by
# the host: 340 os.environ lookups and one torch.cuda.current_stream() per launch were a fifth of it (tools/probes/host_profile.py).
_KNOBS = ("VIRNET_BIAS_FUSED", "VIRNET_ENTRY_FUSED", "VIRNET_T_EMIT", "VIRNET_WX4_EMIT_ROWS", "VIRNET_WX4_ROWS", "VIRNET_CONV_FORM", "VIRNET_WINOGRAD", "VIRNET_WX4_MIN_COUT", "VIRNET_WX4_MIN_TILES", "VIRNET_WX4_MIN_FILL", "VIRNET_WX4_MIN_WGS", "VIRNET_WX4_MIN_SLAB_WGS",
          "VIRNET_RANGE_GUARD", "VIRNET_WGRAD_FORM", "VIRNET_DETERMINISTIC", "VIRNET_KNET_PERSISTENT", "VIRNET_EXIT_FORM", "VIRNET_SFT_MULTI", "VIRNET_ENTRY_FORM", "VIRNET_GUARD_CHECK", "VIRNET_AUTOGRAPH", "VIRNET_AUTOGRAPH_MAX_PIXELS", "VIRNET_AUTOGRAPH_MAX_GRAPHS",
          "VIRNET_TAIL_COMPOSE", "VIRNET_TAIL_COMPOSE_FORM")
class forward_scope:
    """`with ops.forward_scope():` -- the knobs above and the launch stream are read once and held for the block (engine.py wraps every
    inference forward; outside a scope each op reads the environment itself, which is what the kernel-level tests rely on).  The
    snapshot is per THREAD (nat.tls): forwards running in several host threads, each on its own stream, do not see each other's."""

    def __init__(self, form: Optional[str] = None):
        """``form``: override of VIRNET_CONV_FORM for this block only (the range guard's fp32 re-run) -- carried in the thread's
        snapshot, never written to os.environ, so forwards in other threads keep their form."""
        self._form = form

    def __enter__(self):
        tls = nat.tls
        self._prev = (getattr(tls, "scope_env", None), getattr(tls, "stream_cache", None))
        tls.scope_env = {k: os.environ.get(k) for k in _KNOBS}
        self._prev_form = getattr(tls, "form_override", None)
        if self._form is not None:
            tls.form_override = self._form
        if getattr(tls, "form_override", None) is not None:        # (a nested scope keeps the enclosing scope's override)
            tls.scope_env["VIRNET_CONV_FORM"] = tls.form_override
        tls.scope_env["#parsed"] = {}                              # values derived from the knobs, computed once per scope (conv_form, wx4 thresholds)
        tls.stream_cache = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
        return self

    def __exit__(self, *exc):
        nat.tls.scope_env, nat.tls.stream_cache = self._prev
        nat.tls.form_override = self._prev_form
        return False


def _env(name: str, default=None):
    snap = getattr(nat.tls, "scope_env", None)
    if snap is not None:
        v = snap.get(name)
        return default if v is None else v
    return os.environ.get(name, default)


def _parsed(key: str, make):
    """Inside a forward_scope: ``make()`` evaluated once per scope (a single-image forward asks ~9 knob questions per launch);
    outside: evaluated per call, as the kernel-level tests expect."""
    snap = getattr(nat.tls, "scope_env", None)
    if snap is None:
        return make()
    cache = snap["#parsed"]
    v = cache.get(key)
    if v is None:
        v = cache[key] = make()
    return v


def _conv_form_now() -> str:
    form = _env("VIRNET_CONV_FORM")
    if form is None:
        legacy = _env("VIRNET_WINOGRAD")
        form = DEFAULT_CONV_FORM if legacy is None else ("direct" if legacy == "0" else "wino")
    if form not in ("f16x3", "wino", "direct", "bf16", "wx4", "wx4x1"):
        raise ValueError(f"VIRNET_CONV_FORM={form!r}: expected wx4, wx4x1, f16x3, wino, direct or bf16")
    return form


def conv_form() -> str:
    return _parsed("form", _conv_form_now)


_F16_FAMILY = ("f16x3", "bf16", "wx4", "wx4x1")      # the forms whose operands are split-fp16 (bf16 / wx4x1: rounded) on the f16 matrix pipe


def _f16_family() -> bool:
    return conv_form() in _F16_FAMILY


def _wx4_rule():
    return (int(_env("VIRNET_WX4_MIN_COUT", "64")), int(_env("VIRNET_WX4_MIN_TILES", "1")), float(_env("VIRNET_WX4_MIN_FILL", "0.6")),
            _env("VIRNET_DETERMINISTIC", "0") == "1", int(_env("VIRNET_WX4_MIN_WGS", "128")), int(_env("VIRNET_WX4_MIN_SLAB_WGS", "192")))


def wx4_shape_ok(n: int, h: int, w: int, cout: int) -> bool:
    """The Winograd-along-x kernel works on 16 x 32 pixel tiles x 96 channels, ONE workgroup per CU, and a tile takes 2-3x as long as a
    tile of the direct kernel: worth it when the image fills its tiles reasonably AND the launch fills the chip (workgroups =
    images x tiles x channel blocks >= VIRNET_WX4_MIN_WGS, default 128 = half the CUs of an MI355X: measured break-even, tools/bench_conv.py --ab VIRNET_WX4_MIN_WGS=0,100000) -- single small images stay on the
    direct split-fp16 kernel, whose small-grid tile forms give the lower latency (tools/bench_latency.py).  The two forms agree to
    fp32 noise (<= 2e-5 on the network outputs), not bit for bit: with the default rule an image's result can differ in the last bits
    between batch sizes; VIRNET_DETERMINISTIC=1 (older spelling VIRNET_WX4_MIN_WGS=0; or a pinned VIRNET_CONV_FORM=f16x3) restores
    bitwise batch independence (tests/test_e2e_gpu.py holds both).  Inside the Winograd form the library additionally picks the tile
    height per launch size (csrc/conv_f16_wx4.hip: 16-row tiles / one workgroup per CU, or 8-row tiles / two per CU for launches of a
    few hundred workgroups and the 64-channel layers); the deterministic switch pins that as well."""
    min_cout, min_tiles, min_fill, deterministic, min_wgs, min_slab_wgs = _parsed("wx4_rule", _wx4_rule)
    if cout < min_cout:                                     # (64 channels = two-slab workgroups: 5 % ahead of conv_f16 on the SNet convs; 32: behind)
        return False
    th, tw = (h + 15) // 16, (w + 31) // 32
    fill = (h * w) / float(th * 16 * tw * 32)
    if th * tw < min_tiles or fill < min_fill:
        return False
    if deterministic:                                       # one kernel form whatever the batch size (the library pins its tile form too)
        return True
    if n * th * tw * ((cout + 95) // 96) >= min_wgs:
        return True
    # below that: the 8-row form with fewer slabs per workgroup (the library picks the count) when that still gives the chip a round of
    # single-slab work -- the deep levels of a single image (128x128x192: 64 tiles x 6 slabs)
    # (channel counts that are not whole 96-channel blocks -- SISR's 160 / 224 -- would take two or three launches there: the direct
    # kernel's single-slab form does them in one; measured end to end: 256^2 1.27 -> 1.21 ms, SISR x4 1.49 -> 1.56 without this condition)
    return cout % 96 == 0 and n * ((h + 7) // 8) * tw * (cout // 32) >= min_slab_wgs


# An EMITTING launch keeps the Winograd form from this many 16-row workgroups on.  It restates the default of VIRNET_WX4_MIN_WGS
# (_wx4_rule) and does NOT follow the knob's value: the knob only switches this condition off, when it is "0".
WX4_EMIT_MIN_WGS = 128


def conv_form_rule(has_wino: bool, has_f16: bool, has_bf16: bool, has_wx4: bool, transposed: bool, stride: int, cstore_is_cout: bool,
                   n: int, h: int, w: int, c: int, cout: int, res: bool, mask: bool, mul: bool, in_mul: bool,
                   want_raw: bool, want_act: bool, emit: bool) -> Tuple[str, int]:
    """Which kernel family ``conv_mfma`` launches, from plain values: ``(form, emit_rows)`` -- form out of direct | wino | f16x3 | bf16 |
    wx4; emit_rows = the tile height (8 | 16) the Winograd form emits a T image with, 0 for every launch that does not ask it to.
    ``has_*``: the images the PackedWeight carries; ``n, h, w, c``: the input; ``cout``: the weight's; ``res`` .. ``in_mul``: which optional
    operands are given; ``emit``: an emission was asked for.  tests/test_conv_form.py holds it to tests/golden/conv_forms.json."""
    form = "direct"
    plain = not (mask or mul or in_mul)
    if transposed and has_f16 and _f16_family() and plain and want_raw != want_act:
        form = "f16x3"
    elif stride == 2 and not transposed and cstore_is_cout and has_f16 and _f16_family() and not res and plain and not (want_raw and want_act):
        form = "f16x3"
    elif stride == 1 and not transposed and cstore_is_cout:
        want = conv_form()
        if want == "wino" and has_wino:
            form = "wino"
        elif want == "bf16" and has_bf16:
            form = "bf16"
        elif want in ("wx4", "wx4x1") and has_wx4 and wx4_shape_ok(n, h, w, cout):
            form = want                                   # (wx4x1: exactly the launches wx4 would take, one product each)
        elif want in _F16_FAMILY and has_f16 and cout % 32 == 0:
            form = "f16x3"
    if not (emit and form == "wx4"):
        return form, 0
    unpinned = _env("VIRNET_DETERMINISTIC", "0") != "1" and _env("VIRNET_WX4_MIN_WGS") != "0"
    if has_f16 and (in_mul or c < 32 or (n * ((h + 15) // 16) * ((w + 31) // 32) * ((cout + 95) // 96) < WX4_EMIT_MIN_WGS and unpinned)):
        return "f16x3", 0                                # (emission runs the 16-row Winograd tiles only where they fill the chip --
                                                         #  unless the form is pinned: bitwise batch independence)
    if not t_emission_enabled():
        return form, 0
    # emitting tile form of the Winograd kernel: VIRNET_WX4_EMIT_ROWS = 8 | 16
    return form, 8 if _env("VIRNET_WX4_EMIT_ROWS", "8") == "8" and unpinned and _env("VIRNET_WX4_ROWS") != "16" else 16


def pack_wx4_weight(weight: Tensor, *, dgrad: bool = False) -> Tensor:
    """Winograd-along-x split-fp16 image (+ per-row inverse scales) of an OIHW 3x3 weight for virnet_conv_wx4."""
    lib = nat.load()
    return _pack_image(weight, dgrad, lib.virnet_wx4_weight_floats, lib.virnet_pack_wx4_weight, "pack_wx4_weight", "Winograd", "virnet_conv_wx4")


def wx4_last_plan() -> dict:
    """What the calling thread's most recent Winograd-form convolution launched (virnet_conv_wx4_last_plan): tile rows of its first launch,
    whether that was the persistent form, slabs per workgroup, number of launches."""
    out = (C.c_int * 4)()
    nat.load().virnet_conv_wx4_last_plan(out)
    return {"rows": out[0], "persistent": bool(out[1]), "slabs": out[2], "launches": out[3]}


def conv_plan_query(family: int, desc: "nat.ConvDesc", *, emit_rows: int = 0, n_cu: int = 0) -> list:
    """What virnet_conv_wx4 / virnet_conv_f16 (stride 1, stride 2, transposed) would launch for `desc`, without launching and without a
    device (virnet_conv_plan_query; family: nat.PLAN_*): one dict per launch.  Pointers of `desc` are only tested for NULL-ness; n_cu = 0 is
    the current device's CU count.  Raises with the library's message for a descriptor the launch function rejects."""
    lib = nat.load()
    out = (nat.ConvLaunch * 4)()
    n = lib.virnet_conv_plan_query(family, C.byref(desc), emit_rows, n_cu, out, 4)
    if n < 0:
        nat.check(n, "conv_plan_query")
    return [{k: getattr(out[i], k) for k, _ in nat.ConvLaunch._fields_} for i in range(n)]


# ----------------------------------------------------------------------------------------------------------------------
# range guard of the split-fp16 forms (include/virnet_hip.h: virnet_set_range_flag)
# ----------------------------------------------------------------------------------------------------------------------
def range_guard_enabled() -> bool:
    return _env("VIRNET_RANGE_GUARD", "1") != "0"


def range_flag(device: torch.device) -> Optional[Tensor]:
    """The sticky int32 flag of (``device``, calling host thread) -- created zeroed and registered with the library on first use; None
    when the guard is off.  One flag per thread: forwards driven from several host threads (each on its own stream) neither erase nor
    trip each other's flag.  Two streams driven from ONE thread share a flag (a spurious fp32 re-run is the worst case).

    The flags live in the thread's ``threading.local`` (``nat.tls``), exactly like the library's registration (a ``thread_local``
    pointer per device, csrc/api.cpp): both are born on the thread's first guarded forward and die with the OS thread.  (A process-wide
    dict keyed by ``threading.get_ident()`` -- round 4 -- went wrong when a new thread inherited a dead thread's ident: cache hit, no
    registration, its kernels ran with a NULL flag and the guard was silently off)"""
    if not range_guard_enabled():
        return None
    idx = device.index if device.index is not None else torch.cuda.current_device()
    flags = getattr(nat.tls, "range_flags", None)
    if flags is None:
        flags = nat.tls.range_flags = {}
    flag = flags.get(idx)
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
        with torch.cuda.device(idx):
            nat.check(nat.load().virnet_set_range_flag(nat.ptr(flag)), "set_range_flag")
        flags[idx] = flag
    return flag


def range_overflowed(device: torch.device, *, reset: bool = True) -> bool:
    """True when a split-fp16 kernel staged an operand outside fp16's range since the last reset (one device -> host read: it waits for
    the launches enqueued so far)."""
    flag = range_flag(device)
    if flag is None or not bool(flag.item()):
        return False
    if reset:
        flag.zero_()
    return True


def poison_on_flag(flag: Tensor, y: Tensor) -> None:
    """NaN-fill ``y`` on the device when ``flag`` is up (virnet_poison_on_flag): the tail of a replayed graph, see graph.py."""
    nat.check(nat.load().virnet_poison_on_flag(nat.ptr(flag), nat.ptr(y), y.numel(), nat.stream_handle()), "poison_on_flag")


def pack_f16_weight(weight: Tensor, *, dgrad: bool = False, bf16: bool = False) -> Tensor:
    """Split-fp16 image (+ per-row inverse scales) of an OIHW 3x3 weight for virnet_conv_f16 (``dgrad``: of the input-gradient GEMM);
    ``bf16``: the bf16-operand image for virnet_conv_bf16 instead (same size and layout)."""
    lib = nat.load()
    return _pack_image(weight, dgrad, lib.virnet_f16_weight_floats, lib.virnet_pack_bf16_weight if bf16 else lib.virnet_pack_f16_weight,
                       "pack_f16_weight", "split-fp16")


def pack_wino_weight(weight: Tensor, *, dgrad: bool = False) -> Tensor:
    """G g G^T image of an OIHW 3x3 weight for virnet_conv_wino (``dgrad``: of the layer's input-gradient GEMM)."""
    lib = nat.load()
    return _pack_image(weight, dgrad, lib.virnet_wino_weight_floats, lib.virnet_pack_wino_weight, "pack_wino_weight", "Winograd", "the Winograd kernel")


def _pack_image(weight: Tensor, dgrad: bool, floats, pack, what: str, form: str, whole_blocks: Optional[str] = None) -> Tensor:
    """One matrix-pipe image of an OIHW 3x3 weight: ``floats(cin_pad, n_pad)`` sizes it, ``pack`` fills it.  ``whole_blocks``: the name of
    a kernel that stores whole 32-channel blocks only; without it the rows are padded to the next block."""
    weight = weight.detach()
    _dev_check(weight, "weight")
    cout, cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3):
        raise ValueError(f"the {form} form is for 3x3 kernels")
    rows, ks = (cin, cout) if dgrad else (cout, cin)
    if whole_blocks is not None and rows % 32:
        raise ValueError(f"{whole_blocks} stores multiples of 32 channels, got {rows}")
    n_pad = (rows + 31) // 32 * 32            # (rows beyond the real ones are zero; the planar store keeps the real channels)
    cin_pad = (ks + 15) // 16 * 16
    out = torch.empty(floats(cin_pad, n_pad), dtype=torch.float32, device=weight.device)
    nat.check(pack(nat.ptr(weight), int(dgrad), cout, cin, cin_pad, n_pad, nat.ptr(out), nat.stream_handle()), what)
    return out


def _dev_check(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the VIRNet HIP path needs tensors on a ROCm device "
                           f"(no CPU fallback exists; move the module and inputs with .cuda())")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def get_plan(ks: int, stride: int, cin: int, gemm_n: int) -> nat.ConvPlan:
    plan = nat.ConvPlan()
    nat.check(nat.load().virnet_conv_get_plan(ks, stride, cin, gemm_n, C.byref(plan)), "conv_get_plan")
    return plan


def pack_images_rule(kind: str, stride: int, ks: int, cin: int, cout: int) -> Tuple[str, ...]:
    """Which images beside the base fp32 one a packing carries, from plain values and ``conv_form()``: names out of _IMAGE_PACKERS.  ``kind``:
    conv | convt (the 2x2 stride-2 transposed conv) | conv_dgrad (input gradient of a 3x3 conv) | convt_dgrad; ``cin``, ``cout``: the FORWARD
    layer's.  conv_form_rule picks the launch among the images that exist; tests/test_pack_images.py holds this to tests/golden/pack_images.json."""
    form = conv_form()
    f16, cc = form in _F16_FAMILY, {"bf16": ("bf16",), "wx4": ("wx4",), "wx4x1": ("wx4",)}.get(form, ())      # (cc: what the form adds to a C->C layer's split-fp16 image)
    blocks, wide = cout % 32 == 0, cin >= WINO_MIN_CHANNELS              # whole 32-channel output blocks; enough channels for a C->C form
    if kind == "convt":                                                  # UpBlock.upsampler: csrc/conv_f16_convt
        return ("f16_convt",) if f16 and blocks and cin % 16 == 0 else ()
    if kind == "convt_dgrad":                                            # ... its input gradient as a 3x3 stride-2 conv of dy (convt_dgrad)
        return ("s2",) if f16 and cin % 32 == 0 and cout % 16 == 0 else ()
    if kind == "conv_dgrad":                                             # the GEMM's output channels are the layer's cin, its input the cout
        many = cout >= WINO_MIN_CHANNELS                                 # (fewer: few-channel gradient -> features, tail / conv_last backward)
        if cin % 32 or not (f16 or form == "wino" and many):
            return ()
        return ("wino",) if form == "wino" else ("f16",) + (cc if many else ())
    if ks != 3 or stride not in (1, 2):
        return ()
    if stride == 2:                                                      # DownBlock.downsampler: csrc/conv_f16_s2.hip (the stride-1 image)
        return ("f16",) if f16 and blocks and cin % 16 == 0 else ()
    if not f16 or not (blocks or cout <= 32):                            # an fp32 form, or a store neither whole blocks nor planar
        return ("wino",) if form == "wino" and blocks and wide else ()
    # every stride-1 3x3 layer: C->C convs, few-input-channel entry convs (HBM-bound: one 16-channel chunk), through the planar store the exits
    return (("f16",) + (("entry",) if cin <= 8 and blocks and cout <= 96 else ())       # head / DnCNN.conv1: csrc/conv_entry.hip
            + (("exit",) if cout * 9 <= 32 else ())                                      # tail / conv_last / KNet tail: csrc/conv_exit.hip
            + (cc if blocks and wide else ()))


def _pack_small(weight: Tensor, name: str, size: tuple, dims: tuple) -> Tensor:
    """An image with its own sizer and packer in the library: virnet_<name>_weight_floats(*size), virnet_pack_<name>_weight(w, *dims, out)."""
    lib = nat.load()
    out = torch.empty(getattr(lib, f"virnet_{name}_weight_floats")(*size), dtype=torch.float32, device=weight.device)
    nat.check(getattr(lib, f"virnet_pack_{name}_weight")(nat.ptr(weight), *dims, nat.ptr(out), nat.stream_handle()), f"pack_{name}_weight")
    return out


def _pack_convt_dgrad_s2(weight: Tensor) -> "PackedWeight":
    """dx[p][ci] = sum_{a,b,co} dy[2p+(a,b)][co] W[ci][co][a][b] is a 3x3 stride-2 pad-1 conv of dy whose taps (a+1, b+1) hold W and whose
    first row / column are zero: it runs on csrc/conv_f16_s2.hip (split-fp16) straight from the high-res gradient."""
    k3 = torch.zeros(tuple(weight.shape[:2]) + (3, 3), dtype=torch.float32, device=weight.device)
    k3[:, :, 1:, 1:] = weight
    return pack_weight(k3, None, stride=2)


_IMAGE_PACKERS = {      # image name -> (the PackedWeight field it fills, packer(weight, dgrad, cin, cout, plan))
    "wino": ("wino", lambda w, dgrad, cin, cout, plan: pack_wino_weight(w, dgrad=dgrad)),
    "f16": ("f16", lambda w, dgrad, cin, cout, plan: pack_f16_weight(w, dgrad=dgrad)),
    "bf16": ("bf16", lambda w, dgrad, cin, cout, plan: pack_f16_weight(w, dgrad=dgrad, bf16=True)),
    "wx4": ("wx4", lambda w, dgrad, cin, cout, plan: pack_wx4_weight(w, dgrad=dgrad)),
    "entry": ("entry", lambda w, dgrad, cin, cout, plan: _pack_small(w, "entry", (cin, cout), (cout, cin, cout))),
    "exit": ("exit", lambda w, dgrad, cin, cout, plan: _pack_small(w, "exit", (plan.cin_pad,), (cout, cin, plan.cin_pad))),
    "f16_convt": ("f16", lambda w, dgrad, cin, cout, plan: _pack_small(w, "f16_convt", (cin, cout), (cout, cin))),
    "s2": ("s2", lambda w, dgrad, cin, cout, plan: _pack_convt_dgrad_s2(w))}


def pack_weight(weight: Tensor, bias: Optional[Tensor], *, transposed: bool = False, stride: int = 1, dgrad: bool = False) -> PackedWeight:
    """Pack an OIHW conv weight or an IOHW (k=2,s=2) transposed-conv weight for virnet_conv_mfma, with the images pack_images_rule names.  ``dgrad=True``
    packs the INPUT-GRADIENT GEMM of the same layer instead (flipped/transposed 3x3 taps, or the pointwise GEMM over the space-to-depth gradient for the
    transposed conv); the result is used like a forward weight with cout = forward cin."""
    lib = nat.load()
    weight = weight.detach()
    _dev_check(weight, "weight")
    kind = ("convt" if transposed else "conv") + ("_dgrad" if dgrad else "")
    (cin, cout), (kh, kw) = weight.shape[:2] if transposed else weight.shape[1::-1], weight.shape[2:]
    if kind == "conv_dgrad" and (kh, kw) != (3, 3):
        raise ValueError("dgrad packing handles 3x3 convs and the 2x2 transposed conv")
    if kind == "convt" and (kh, kw) != (2, 2):
        raise ValueError("only ConvTranspose2d(k=2, s=2) is on the path (networks/AttResUNet.py:80)")
    if kind == "conv" and (kh != kw or kh not in (1, 3)):
        raise ValueError(f"unsupported kernel {kh}x{kw}")
    # the library's kind code, its kernel side, the GEMM's taps per side, its (stride, input channels, output channels), what the packing calls cout / cin
    code, ks, gemm_ks, gemm, pw_cout, pw_cin = {
        "conv": (0, kh, kh, (stride, cin, cout), cout, cin), "convt": (1, 2, 1, (1, cin, 4 * cout), cout, cin),
        "conv_dgrad": (2, 3, 3, (1, cout, cin), cin, cout), "convt_dgrad": (3, 2, 1, (1, 4 * cout, cin), cin, 4 * cout)}[kind]
    plan = get_plan(gemm_ks, *gemm)
    out = torch.empty(lib.virnet_packed_weight_floats(gemm_ks, plan.cin_pad, plan.n_pad), dtype=torch.float32, device=weight.device)
    nat.check(lib.virnet_pack_weight(nat.ptr(weight), code, cout, cin, ks, plan.cin_pad, plan.n_pad, plan.nrep, nat.ptr(out),
                                     nat.stream_handle()), "pack_weight(dgrad)" if dgrad else "pack_weight")
    b = None if bias is None or dgrad else bias.detach()
    if b is not None:
        _dev_check(b, "bias")
    pw = PackedWeight(out, b, gemm_ks, pw_cout, pw_cin, plan.cin_pad, plan.n_pad, plan.nrep, kind == "convt")
    for name in pack_images_rule(kind, stride, kh, cin, cout):
        field, pack = _IMAGE_PACKERS[name]
        setattr(pw, field, pack(weight, dgrad, cin, cout, plan))
    return pw


@dataclass
class TImage:
    """Channel-major fp16 hi|lo (or bf16) image of an NHWC tensor -- the operand layout of the f16-pipe weight gradient
    (csrc/wgrad_f16.hip) -- as written by ``virnet_chsplit`` or emitted by a convolution's epilogue; ``db``: the tensor's channel sums
    (bias gradient) when they were asked for."""
    buf: Tensor
    n: int
    h: int
    w: int
    c: int
    bf16: bool
    db: Optional[Tensor] = None
    pooled: bool = False
    # channel sums still pending as per-workgroup partials (the emitting conv left them; the consuming weight gradient reduces them in
    # its own reduction launch -- or bias_sums() on demand): col[(cb * nblk + blk) * 32 + ch], ncol = channels asked for
    col: Optional[Tensor] = None
    nblk: int = 0
    ncol: int = 0
    col_gen: Optional[Tuple[int, int]] = None   # (workspace turn, generation) of `col`: the partials live in one of two alternating workspaces

    def col_fresh(self) -> None:
        """The pending partials sit in a per-thread workspace that the SECOND-next emitting conv overwrites (conv_mfma: emit_col0 / emit_col1):
        a backward ordering that keeps two images pending would read another image's sums.  Checked wherever the partials are consumed."""
        if self.col is not None and self.col_gen is not None:
            turn, gen = self.col_gen
            now = getattr(nat.tls, "emit_col_gen", {}).get(turn)
            if now != gen:
                raise RuntimeError(f"TImage: the bias-gradient partials of this image were overwritten (workspace {turn}: generation {gen} -> {now}): "
                                   "more than one other emitting convolution ran before its weight gradient consumed them")

    def bias_sums(self) -> Optional[Tensor]:
        """The tensor's channel sums (bias gradient), reducing the pending partials if nothing has done so yet."""
        self.col_fresh()
        if self.db is None and self.col is not None:
            self.db = _zeros(self.ncol, self.col.device)
            nat.check(nat.load().virnet_colpart_reduce(nat.ptr(self.col), nat.ptr(self.db), self.nblk, self.c // 32, self.ncol, nat.stream_handle()),
                      "colpart_reduce")
            self.col = None
        return self.db


_T_POOL: dict = {}
T_POOL_MAX_BYTES = int(os.environ.get("VIRNET_T_POOL_MB", "8192")) << 20     # recycled T buffers kept across steps (a training step at configs[4]'s shape holds ~1.6 GB)


def _t_pool_trim() -> None:
    """Keep the recycled buffers under T_POOL_MAX_BYTES: geometries are dropped least-recently-released first (a long-lived process that
    sees many patch sizes would otherwise keep one set per geometry for ever -- VERDICT r04 weak #11)."""
    total = sum(b.numel() for free in _T_POOL.values() for b in free)
    for key in list(_T_POOL):
        if total <= T_POOL_MAX_BYTES:
            break
        total -= sum(b.numel() for b in _T_POOL[key])
        del _T_POOL[key]


def t_acquire(n: int, h: int, w: int, c: int, bf16: bool, device: torch.device) -> TImage:
    """A T buffer whose pad rows / segments are zero: emitting kernels write only the image rows, so buffers of one geometry are
    recycled (``t_release``) instead of being zero-filled per use (a fill is 40 % of the re-layout pass the emission replaces)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, n, h, w, c)
    free = _T_POOL.get(key)
    buf = free.pop() if free else torch.zeros(nat.load().virnet_chsplit_bytes(n, h, w, c), dtype=torch.uint8, device=device)
    return TImage(buf, n, h, w, c, bf16, None, True)


def t_release(t: Optional[TImage]) -> None:
    if t is not None and t.pooled and t.buf is not None:
        dev = t.buf.device
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, t.n, t.h, t.w, t.c)
        free = _T_POOL.pop(key, [])                 # (re-inserted at the end: dict order = least recently released first)
        free.append(t.buf)
        _T_POOL[key] = free
        t.buf = None
        if len(free) == 1 and len(_T_POOL) > 1:      # a geometry (re)entered the pool
            _t_pool_trim()


class zero_arena:
    """`with ops.zero_arena(n, device):` -- the small zero-initialised fp32 vectors the block asks for (bias gradients: ~45 per training
    step, each a fill launch of its own otherwise) are carved out of ONE zeroed buffer; beyond its size `torch.zeros` takes over."""

    def __init__(self, nfloats: int, device: torch.device):
        self.n, self.device = int(nfloats), device

    def __enter__(self):
        self._prev = getattr(nat.tls, "zero_arena", None)
        nat.tls.zero_arena = [torch.zeros(self.n, dtype=torch.float32, device=self.device), 0] if self.n > 0 else None
        return self

    def __exit__(self, *exc):
        nat.tls.zero_arena = self._prev
        return False


def _zeros(n: int, device: torch.device) -> Tensor:
    ar = getattr(nat.tls, "zero_arena", None)
    if ar is not None and ar[0].device == device and ar[1] + n <= ar[0].numel():
        out = ar[0][ar[1]:ar[1] + n]
        ar[1] += n
        return out
    return torch.zeros(n, dtype=torch.float32, device=device)


def t_pool_clear() -> None:
    """Drop the recycled T buffers (they are grow-only: one set per geometry the training step has seen)."""
    _T_POOL.clear()


def t_emission_enabled() -> bool:
    """VIRNET_T_EMIT=0 keeps the separate re-layout passes (A/B runs)."""
    return _env("VIRNET_T_EMIT", "1") != "0"


def conv_mfma(x: Tensor, pw: PackedWeight, *, stride: int = 1, res: Optional[Tensor] = None,
              mul: Optional[Tensor] = None, add: Optional[Tensor] = None, want_raw: bool = True,
              want_act: bool = False, slope: float = 0.2, in_slope: Optional[float] = None,
              in_mul: Optional[Tensor] = None, in_add: Optional[Tensor] = None, mask: Optional[Tensor] = None,
              mask_slope: float = 0.2, out_channels: Optional[int] = None, emit: Optional[dict] = None, thin_wx4: bool = False):
    """NHWC conv (or transposed conv when ``pw.transposed``) -> (raw, act), each NHWC or None.

    ``in_slope`` (with optional per-(image, channel) ``in_mul``/``in_add``): the conv consumes
    ``leaky_relu(x*in_mul+in_add, in_slope)`` -- the pre-activation of AttResUNet.py:55 -- applied while x is staged.

    ``emit`` (training step) = dict(act=None | slope, colsum=None | channels): the conv is asked to emit, next to its stored tensor,
    that tensor's T image (of ``lrelu(y, act)`` when ``act`` is given) and optionally its channel sums; the call then returns
    ``(raw, act, TImage | None)`` -- None when this launch cannot emit (form / shape), the caller re-lays the tensor itself.

    ``thin_wx4`` (one call site: the composed 96 -> 32 conv of engine.rnet_forward): a single-slab launch that the rule sends to the
    direct kernel for its channel count alone takes the Winograd form where a 64-channel layer of the same shape would."""
    _dev_check(x, "x")
    n, h, w, c = x.shape
    if c != pw.cin_pad:
        raise ValueError(f"x has {c} channels, packed weight expects {pw.cin_pad}")
    if pw.transposed:
        oh, ow, epi = 2 * h, 2 * w, nat.EPI_CONVT
    else:
        oh, ow, epi = h // stride, w // stride, nat.EPI_NHWC
    cstore = pw.cout if out_channels is None else out_channels      # backward of thin layers: store the 32-padded rows
    raw = torch.empty((n, oh, ow, cstore), dtype=torch.float32, device=x.device) if want_raw else None
    act = torch.empty((n, oh, ow, cstore), dtype=torch.float32, device=x.device) if want_act else None
    if mask is not None:
        _dev_check(mask, "mask")
        if tuple(mask.shape) != (n, oh, ow, cstore):
            raise ValueError(f"mask shape {tuple(mask.shape)} != {(n, oh, ow, cstore)}")
    for t, nm in ((res, "res"), (mul, "mul"), (add, "add"), (in_mul, "in_mul"), (in_add, "in_add")):
        if t is not None:
            _dev_check(t, nm)
    if in_mul is not None and (tuple(in_mul.shape) != (n, c) or tuple(in_add.shape) != (n, c)):
        raise ValueError(f"in_mul/in_add must be [{n}, {c}]")
    if res is not None and tuple(res.shape) != (n, oh, ow, cstore):
        raise ValueError(f"res shape {tuple(res.shape)} != {(n, oh, ow, cstore)}")
    form, rows = conv_form_rule(pw.wino is not None, pw.f16 is not None, pw.bf16 is not None, pw.wx4 is not None, pw.transposed, stride,
                                cstore == pw.cout, n, h, w, c, pw.cout, res is not None, mask is not None, mul is not None, in_mul is not None,
                                want_raw, want_act, emit is not None)
    if thin_wx4 and form == "f16x3" and emit is None and pw.wx4 is not None and conv_form() == "wx4" and wx4_shape_ok(n, h, w, max(pw.cout, 64)):
        form = "wx4"
    _, image, what = _CONV_FORMS[form]
    wimg = getattr(pw, image)
    d = nat.ConvDesc(x=nat.ptr(x), wpack=nat.ptr(wimg), bias=nat.ptr(pw.bias), res=nat.ptr(res), mul=nat.ptr(mul),
                     add=nat.ptr(add), mask=nat.ptr(mask), mask_slope=mask_slope, in_mul=nat.ptr(in_mul), in_add=nat.ptr(in_add),
                     y_raw=nat.ptr(raw), y_act=nat.ptr(act), n=n, h=h, w=w, cin_pad=c, cout=cstore, n_pad=pw.n_pad, nrep=pw.nrep, ks=pw.ks,
                     stride=stride, epi=epi, nchw_op=0, crop_h=0, crop_w=0, res_sf=1, in_act=int(in_slope is not None),
                     in_slope=0.0 if in_slope is None else in_slope, slope=slope, clamp_lo=0.0, clamp_hi=0.0)
    # algorithmic FLOPs = 2*MAC over the REAL channels; the transposed conv does 4*cout columns per input pixel
    flops = 2.0 * n * h * w * pw.cin_real * pw.cout * 4 if pw.transposed else 2.0 * n * oh * ow * pw.cin_real * pw.cout * pw.ks ** 2
    if emit is None:
        _launch_conv(d, flops, what, form)
        return raw, act
    require_trainable_form("a convolution that emits a T image")
    timg, nblk = None, C.c_int(0)
    if (t_emission_enabled() and form in _F16_FAMILY and not pw.transposed and stride == 1
            and nat.load().virnet_conv_emit_ok(C.byref(d), (2 if rows == 8 else 1) if form == "wx4" else 0, C.byref(nblk))):
        timg = t_acquire(n, oh, ow, cstore, form == "bf16", x.device)
        col = None
        ncol = emit.get("colsum")
        if ncol is not None:
            # two alternating buffers: the partials wait for the weight gradient that consumes this image, and at most one other
            # emitting conv runs before it (train.py: dgrad conv -> wgrad of the previous conv -> next dgrad conv)
            turn = nat.tls.emit_col_turn = getattr(nat.tls, "emit_col_turn", 0) ^ 1          # (per host thread, like the workspaces' streams)
            col = _workspace("emit_col%d" % turn, nblk.value * cstore * 4, x.device)
            gens = getattr(nat.tls, "emit_col_gen", None)
            if gens is None:
                gens = nat.tls.emit_col_gen = {}
            gens[turn] = gens.get(turn, 0) + 1
            timg.col, timg.nblk, timg.ncol, timg.col_gen = col, nblk.value, ncol, (turn, gens[turn])
        slope_t = emit.get("act")
        te = nat.TEmit(t_out=nat.ptr(timg.buf), col=nat.ptr(col), act=int(slope_t is not None), slope=0.0 if slope_t is None else slope_t,
                       bf16=int(form == "bf16"), rows=rows)
        _launch_conv(d, flops, what + "(+T)", form, te)
        if col is not None and _env("VIRNET_BIAS_FUSED", "1") == "0":
            timg.bias_sums()                             # (A/B knob: reduce the partials now, in a launch of their own)
    else:
        _launch_conv(d, flops, what, form)
    return raw, act, timg


def _planar_out(x: Tensor, pw: PackedWeight, crop_hw: Tuple[int, int], res: Optional[Tensor], res_sf: int, fits: bool, why: str):
    """What the three planar-store convolutions start with: the checks of ``x``, of the channel count (``fits``: the op's own condition on
    the packing; ``why``: its half of the error text), of ``res``, and the output -> (n, h, w, c, crop h, crop w, out)."""
    _dev_check(x, "x")
    n, h, w, c = x.shape
    if c != pw.cin_pad or not fits:
        raise ValueError(f"x has {c} channels" + why.format(cin_pad=pw.cin_pad, cout=pw.cout))
    ch, cw = crop_hw
    out = torch.empty((n, pw.cout, ch, cw), dtype=torch.float32, device=x.device)
    if res is not None:
        _dev_check(res, "res")
        if tuple(res.shape) != (n, pw.cout, ch // res_sf, cw // res_sf):
            raise ValueError(f"res shape {tuple(res.shape)} != {(n, pw.cout, ch // res_sf, cw // res_sf)}")
    return n, h, w, c, ch, cw, out


def conv_mfma_nchw(x: Tensor, pw: PackedWeight, crop_hw: Tuple[int, int], *, op: int = nat.NCHW_PLAIN,
                   res: Optional[Tensor] = None, res_sf: int = 1, clamp: Tuple[float, float] = (0.0, 0.0)) -> Tensor:
    """Thin-output 3x3 conv with planar (NCHW) store, crop and fused `+res` / `exp(clamp(.))` epilogue.

    With ``res_sf`` > 1 ``res`` is the low-resolution image and is added through a nearest up-sampling."""
    n, h, w, c, ch, cw, out = _planar_out(x, pw, crop_hw, res, res_sf, True, ", packed weight expects {cin_pad}")
    d = nat.ConvDesc(x=nat.ptr(x), wpack=nat.ptr(pw.w), bias=nat.ptr(pw.bias), res=nat.ptr(res), mul=0, add=0, mask=0,
                     mask_slope=0.0, in_mul=0, in_add=0, in_act=0, in_slope=0.0, y_raw=nat.ptr(out), y_act=0, n=n, h=h, w=w, cin_pad=c, cout=pw.cout, n_pad=pw.n_pad,
                     nrep=pw.nrep, ks=pw.ks, stride=1, epi=nat.EPI_NCHW, nchw_op=op, crop_h=ch, crop_w=cw,
                     res_sf=res_sf, slope=0.0, clamp_lo=clamp[0], clamp_hi=clamp[1])
    _launch_conv(d, 2.0 * n * h * w * pw.cin_real * pw.cout * pw.ks ** 2, "conv_mfma(nchw)")
    return out


def conv_f16_nchw(x: Tensor, pw: PackedWeight, crop_hw: Tuple[int, int], *, op: int = nat.NCHW_PLAIN,
                  res: Optional[Tensor] = None, res_sf: int = 1, clamp: Tuple[float, float] = (0.0, 0.0), z_add: Optional[Tensor] = None) -> Tensor:
    """Few-output-channel (<= 32) 3x3 conv on the split-fp16 kernel with planar (NCHW) store, crop and fused `+res` / `exp(clamp(.))`.

    ``z_add`` (taps-as-rows kernel only): [N, H, W, 32] additive partial map of the rows z[(channel, tap)] -- the composed tail of
    ``compose_exit_weight`` (virnet_conv_exit_add)."""
    n, h, w, c, ch, cw, out = _planar_out(x, pw, crop_hw, res, res_sf, pw.f16 is not None and pw.cout <= 32,
                                          " / weight has no split-fp16 image for a planar store (cin_pad {cin_pad}, cout {cout})")
    lib = nat.load()
    # taps-as-rows exit kernel (csrc/conv_exit.hip) when the (channel, tap) pairs fit one MFMA block; VIRNET_EXIT_FORM=f16 keeps conv_f16's planar form
    use_exit = pw.exit is not None and _env("VIRNET_EXIT_FORM", "rows") != "f16"
    d = nat.ConvDesc(x=nat.ptr(x), wpack=nat.ptr(pw.exit if use_exit else pw.f16), bias=nat.ptr(pw.bias), res=nat.ptr(res), mul=0, add=0, mask=0,
                     mask_slope=0.0, in_mul=0, in_add=0, in_act=0, in_slope=0.0, y_raw=nat.ptr(out), y_act=0, n=n, h=h, w=w, cin_pad=c, cout=pw.cout,
                     n_pad=32, nrep=1, ks=3, stride=1, epi=nat.EPI_NCHW, nchw_op=op, crop_h=ch, crop_w=cw,
                     res_sf=res_sf, slope=0.0, clamp_lo=clamp[0], clamp_hi=clamp[1])
    flops = 2.0 * n * h * w * pw.cin_real * pw.cout * 9
    if z_add is not None:
        _dev_check(z_add, "z_add")
        if not use_exit or c not in (64, 96) or tuple(z_add.shape) != (n, h, w, 32):
            raise ValueError(f"z_add {tuple(z_add.shape)}: the additive map is [N, H, W, 32] for the taps-as-rows exit kernel with 64 or 96 "
                             f"input channels (x {tuple(x.shape)}, rows form {use_exit})")
        _timed_call(lib.virnet_conv_exit_add, (C.byref(d), nat.ptr(z_add)), "conv_exit(z_add)", ("exit", pw.cout), flops)
    elif use_exit:
        _timed_call(lib.virnet_conv_exit, (C.byref(d),), "conv_exit", ("exit", pw.cout), flops)
    else:
        _timed_call(lib.virnet_conv_f16, (C.byref(d),), "conv_f16(nchw)", ("f16x3", pw.cout), flops)
    return out


def compose_exit_weight(w2: Tensor, b2: Optional[Tensor], w_exit: Tensor) -> PackedWeight:
    """The exit conv ``w_exit`` ([ce, cm, 3, 3], ce * 9 <= 32) composed with the 3x3 conv (``w2`` [cm, ci, 3, 3], ``b2``) that feeds it
    WITHOUT an activation in between, as an ordinary packed ci -> 32 3x3 weight (virnet_compose_exit_weight: fp64 accumulation, rounded
    once; rows ce * 9 .. 31 zero): ``conv_mfma(t, .)`` is the additive map ``z_add`` of ``conv_f16_nchw`` -- the exit's taps-as-rows GEMM
    z = A y is pointwise, so it distributes over y = r + conv(t; w2) + b2 exactly, zero padding of y included."""
    w2, w_exit = w2.detach(), w_exit.detach()
    b2 = None if b2 is None else b2.detach()
    for t, nm in ((w2, "w2"), (b2, "b2"), (w_exit, "w_exit")):
        if t is not None:
            _dev_check(t, nm)
    ce, cm = w_exit.shape[:2]
    if tuple(w_exit.shape[2:]) != (3, 3) or tuple(w2.shape[2:]) != (3, 3) or w2.shape[0] != cm or ce * 9 > 32:
        raise ValueError(f"compose_exit_weight: exit {tuple(w_exit.shape)} over conv {tuple(w2.shape)}: 3x3 kernels, matching channels and "
                         f"at most 3 exit channels")
    ci = w2.shape[1]
    wc = torch.empty((32, ci, 3, 3), dtype=torch.float32, device=w2.device)
    bc = torch.empty(32, dtype=torch.float32, device=w2.device)
    nat.check(nat.load().virnet_compose_exit_weight(nat.ptr(w2), nat.ptr(b2), nat.ptr(w_exit), ce, cm, ci, nat.ptr(wc), nat.ptr(bc),
                                                    nat.stream_handle()), "compose_exit_weight")
    return pack_weight(wc, bc)


def pack_thin_weight(weight: Tensor, bias: Optional[Tensor]) -> PackedWeight:
    """Pack an OIHW 3x3 weight with 1..4 output channels for virnet_conv3x3_thin."""
    lib = nat.load()
    weight = weight.detach()
    _dev_check(weight, "weight")
    cout, cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or not 1 <= cout <= 4:
        raise ValueError(f"thin conv handles 3x3 kernels with 1..4 output channels, got {tuple(weight.shape)}")
    c_pad = (cin + 15) // 16 * 16
    out = torch.empty(lib.virnet_thin_weight_floats(c_pad), dtype=torch.float32, device=weight.device)
    nat.check(lib.virnet_pack_thin_weight(nat.ptr(weight), cout, cin, c_pad, nat.ptr(out), nat.stream_handle()), "pack_thin_weight")
    b = None
    if bias is not None:
        b = bias.detach()
        _dev_check(b, "bias")
    return PackedWeight(out, b, 3, cout, cin, c_pad, 4, 0, False)


def conv3x3_thin(x: Tensor, pw: PackedWeight, crop_hw: Tuple[int, int], *, op: int = nat.NCHW_PLAIN,
                 res: Optional[Tensor] = None, res_sf: int = 1, clamp: Tuple[float, float] = (0.0, 0.0)) -> Tensor:
    """3x3 conv to 1..4 channels, planar (NCHW) store with crop and fused `+res` / `exp(clamp(.))` (bandwidth-bound kernel)."""
    n, h, w, c, ch, cw, out = _planar_out(x, pw, crop_hw, res, res_sf, pw.nrep == 0, " / weight is not a thin pack (expects {cin_pad})")
    d = nat.ThinDesc(x=nat.ptr(x), wpack=nat.ptr(pw.w), bias=nat.ptr(pw.bias), res=nat.ptr(res), y=nat.ptr(out), n=n, h=h, w=w,
                     c=c, cout=pw.cout, crop_h=ch, crop_w=cw, op=op, res_sf=res_sf, clamp_lo=clamp[0], clamp_hi=clamp[1])
    _timed_call(nat.load().virnet_conv3x3_thin, (C.byref(d),), "conv3x3_thin", ("thin", 3, 1, pw.cout), 2.0 * n * h * w * pw.cin_real * pw.cout * 9)
    return out


def conv_planar(x: Tensor, conv, crop_hw: Tuple[int, int], **kw) -> Tensor:
    """The network exits (``conv``: a networks.params conv layer with few output channels): 3x3 conv with planar (NCHW) store on the
    split-fp16 kernel (one slab) in that family of forms, else the bandwidth-bound kernel for <= 4 output channels and the fp32 MFMA
    kernel beyond; ``kw`` as for those three."""
    if _f16_family() and conv.cout <= 32:
        return conv_f16_nchw(x, conv.packed(), crop_hw, **kw)
    if conv.cout <= 4:
        return conv3x3_thin(x, conv.packed_thin(), crop_hw, **kw)
    return conv_mfma_nchw(x, conv.packed(), crop_hw, **kw)


def pack_input(x: Tensor, hp: int, wp: int, *, sf: int = 1, vec: Optional[Tensor] = None,
               map_: Optional[Tensor] = None, map_sf: int = 1, map_sqrt: bool = False, zero_pad: bool = False) -> Tensor:
    """NCHW image (+ per-image vector / per-pixel map) -> [N, hp, wp, 16] NHWC records (up-sample, reflect pad, concat)."""
    _dev_check(x, "x")
    n, c0, h, w = x.shape
    ev = 0 if vec is None else vec.shape[1]
    em, mh, mw = (0, 0, 0) if map_ is None else map_.shape[1:]
    if vec is not None:
        _dev_check(vec, "vec")
    if map_ is not None:
        _dev_check(map_, "map")
    out = torch.empty((n, hp, wp, 16), dtype=torch.float32, device=x.device)
    d = nat.PackDesc(x=nat.ptr(x), vec=nat.ptr(vec), map=nat.ptr(map_), out=nat.ptr(out), n=n, c0=c0, h=h, w=w, sf=sf,
                     ev=ev, em=em, mh=mh, mw=mw, msf=map_sf, map_sqrt=int(map_sqrt), hp=hp, wp=wp, zero_pad=int(zero_pad))
    nat.check(nat.load().virnet_pack_input(C.byref(d), nat.stream_handle()), "pack_input")
    return out


def conv_entry(x: Tensor, pw: PackedWeight, hp: int, wp: int, *, sf: int = 1, vec: Optional[Tensor] = None, map_: Optional[Tensor] = None,
               map_sf: int = 1, map_sqrt: bool = False, want_act: bool = False, slope: float = 0.2) -> Tensor:
    """The network entry as ONE launch: ``conv3x3(pack_input(x, hp, wp, ...))`` (AttResUNet.head AttResUNet.py:153-155, DnCNN.conv1
    DnCNN.py:38) with the 16-channel record gathered from the NCHW image / vector / map inside the conv's staging
    (``virnet_conv_f16_entry``) -- no packed tensor, one launch less.  Returns the NHWC output (raw, or ``lrelu(., slope)`` with
    ``want_act``).  Forms or channel counts without the fused kernel take the two-launch path; same bits either way."""
    _dev_check(x, "x")
    n, c0, h, w = x.shape
    ev = 0 if vec is None else vec.shape[1]
    em, mh, mw = (0, 0, 0) if map_ is None else map_.shape[1:]
    kw = dict(want_raw=not want_act, want_act=want_act, slope=slope)
    if not (_f16_family() and pw.f16 is not None and pw.cin_pad == 16 and pw.cout % 32 == 0 and c0 + ev + em <= 8
            and _env("VIRNET_ENTRY_FUSED", "1") != "0"):
        rec = pack_input(x, hp, wp, sf=sf, vec=vec, map_=map_, map_sf=map_sf, map_sqrt=map_sqrt)
        raw, act = conv_mfma(rec, pw, **kw)
        return act if want_act else raw
    for t, nm in ((vec, "vec"), (map_, "map")):
        if t is not None:
            _dev_check(t, nm)
    out = torch.empty((n, hp, wp, pw.cout), dtype=torch.float32, device=x.device)
    # the store-bound entry kernel (csrc/conv_entry.hip) when its weight image exists; VIRNET_ENTRY_FORM=f16 keeps round 4's conv_f16 ENT form
    # (bitwise = pack_input + conv_f16; the two agree to fp32 rounding)
    use_entry = pw.entry is not None and c0 + ev + em == pw.cin_real and _env("VIRNET_ENTRY_FORM", "rows") != "f16"
    d = nat.ConvDesc(x=nat.ptr(x), wpack=nat.ptr(pw.entry if use_entry else pw.f16), bias=nat.ptr(pw.bias), res=0, mul=0, add=0, mask=0, mask_slope=0.0, in_mul=0, in_add=0,
                     y_raw=0 if want_act else nat.ptr(out), y_act=nat.ptr(out) if want_act else 0, n=n, h=hp, w=wp, cin_pad=16, cout=pw.cout,
                     n_pad=pw.n_pad, nrep=pw.nrep, ks=3, stride=1, epi=nat.EPI_NHWC, nchw_op=0, crop_h=0, crop_w=0, res_sf=1, in_act=0,
                     in_slope=0.0, slope=slope, clamp_lo=0.0, clamp_hi=0.0)
    e = nat.PackDesc(x=nat.ptr(x), vec=nat.ptr(vec), map=nat.ptr(map_), out=0, n=n, c0=c0, h=h, w=w, sf=sf, ev=ev, em=em, mh=mh, mw=mw,
                     msf=map_sf, map_sqrt=int(map_sqrt), hp=hp, wp=wp, zero_pad=0)
    lib = nat.load()
    flops = 2.0 * n * hp * wp * pw.cin_real * pw.cout * 9
    if use_entry:
        _timed_call(lib.virnet_conv_entry, (C.byref(d), C.byref(e)), "conv_entry", ("entry", pw.cout), flops)
    else:
        _timed_call(lib.virnet_conv_f16_entry, (C.byref(d), C.byref(e)), "conv_f16_entry", ("f16x3", pw.cout), flops)
    return out


GAP_MEAN, GAP_EXPCLAMP, GAP_KINFO = nat.GAP_MEAN, nat.GAP_EXPCLAMP, nat.GAP_KINFO


def gap_nchw(x: Tensor, finish: int = GAP_MEAN, clamp: Tuple[float, float] = (0.0, 0.0)) -> Tensor:
    """Planar global average pool [N,C,H,W] -> [N,C] with the call site's finishing op fused."""
    _dev_check(x, "x")
    n, c, h, w = x.shape
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    nat.check(nat.load().virnet_gap_nchw(nat.ptr(x), nat.ptr(out), n, c, h, w, finish, clamp[0], clamp[1],
                                         nat.stream_handle()), "gap_nchw")
    return out


def conv_head_s4(x: Tensor, weight: Tensor) -> Tensor:
    """KernelNet.head: 9x9 stride-4 pad-4 conv without bias, NCHW in -> NHWC out."""
    _dev_check(x, "x")
    weight = weight.detach()
    _dev_check(weight, "weight")
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    if tuple(weight.shape[1:]) != (cin, 9, 9):
        raise ValueError(f"head weight {tuple(weight.shape)} does not match a 9x9 conv on {cin} channels")
    oh, ow = (h - 1) // 4 + 1, (w - 1) // 4 + 1
    out = torch.empty((n, oh, ow, cout), dtype=torch.float32, device=x.device)
    nat.check(nat.load().virnet_conv_head_s4(nat.ptr(x), nat.ptr(weight), nat.ptr(out), n, cin, h, w, cout,
                                             nat.stream_handle()), "conv_head_s4")
    return out


def conv_head_s4_wgrad(x: Tensor, dy: Tensor, cout: int) -> Tensor:
    """Weight gradient [cout, cin, 9, 9] of KernelNet.head from the NCHW input and the NHWC output gradient."""
    _dev_check(x, "x"); _dev_check(dy, "dy")
    n, cin, h, w = x.shape
    oh, ow = (h - 1) // 4 + 1, (w - 1) // 4 + 1
    if tuple(dy.shape) != (n, oh, ow, cout):
        raise ValueError(f"dy shape {tuple(dy.shape)} != {(n, oh, ow, cout)}")
    dw = torch.empty((cout, cin, 9, 9), dtype=torch.float32, device=x.device)
    nat.check(nat.load().virnet_conv_head_s4_wgrad(nat.ptr(x), nat.ptr(dy), nat.ptr(dw), n, cin, h, w, cout, nat.stream_handle()),
              "conv_head_s4_wgrad")
    return dw


def conv_head_s4_dgrad(dy: Tensor, weight: Tensor, hw: Tuple[int, int]) -> Tensor:
    """Input gradient [N, cin, h, w] (NCHW) of KernelNet.head from the NHWC output gradient ``dy`` [N, oh, ow, cout]."""
    _dev_check(dy, "dy")
    weight = weight.detach()
    _dev_check(weight, "weight")
    n, oh, ow, cout = dy.shape
    h, w = hw
    if tuple(weight.shape[0:1]) != (cout,) or tuple(weight.shape[2:]) != (9, 9) or cout % 4:
        raise ValueError(f"head weight {tuple(weight.shape)} does not match a 9x9 conv to {cout} channels")
    if (oh, ow) != ((h - 1) // 4 + 1, (w - 1) // 4 + 1):
        raise ValueError(f"dy {tuple(dy.shape)} is not the stride-4 output of a {h}x{w} image")
    if weight.device != dy.device:
        raise ValueError(f"weight on {weight.device}, dy on {dy.device}")
    cin = weight.shape[1]
    dx = torch.empty((n, cin, h, w), dtype=torch.float32, device=dy.device)
    nat.check(nat.load().virnet_conv_head_s4_dgrad(nat.ptr(dy), nat.ptr(weight), nat.ptr(dx), n, cin, h, w, cout, nat.stream_handle()),
              "conv_head_s4_dgrad")
    return dx


def image_grad(hw: Tuple[int, int], c0: int, *, n: Optional[int] = None, dres: Optional[Tensor] = None, sf: int = 1,
               ga: Optional[Tensor] = None, wa: Optional[Tensor] = None, gb: Optional[Tensor] = None, wb: Optional[Tensor] = None,
               into: Optional[Tensor] = None) -> Tensor:
    """Image gradient [N, c0, h, w] of the network's entry convolutions (csrc/image_grad.hip, virnet_image_grad): the residual ``dres``
    [N, c0, sf*h, sf*w] folded over the nearest x``sf`` up-sampling, plus the input gradient of a 3x3 conv with weights ``wa`` whose
    output gradient ``ga`` [N, hp, wp, ca] sits on records up-sampled by ``sf`` and reflect-padded to hp x wp, plus that of a 3x3 conv with
    weights ``wb`` at h x w (``gb`` [N, h, w, cb], zero padding).  Every term is optional; ``into``: accumulate into that tensor."""
    h, w = hw
    srcs = [t for t in (dres, ga, gb, into) if t is not None]
    if n is None:
        if not srcs:
            raise ValueError("image_grad: no term and no batch size")
        n = srcs[0].shape[0]
    for t, nm in ((dres, "dres"), (ga, "ga"), (wa, "wa"), (gb, "gb"), (wb, "wb"), (into, "into")):
        if t is not None:
            _dev_check(t, nm)
    if not 1 <= c0 <= 4 or sf < 1:
        raise ValueError(f"image_grad: c0={c0} (1..4), sf={sf}")
    dev = srcs[0].device if srcs else None
    if any(t.device != dev for t in srcs + [t for t in (wa, wb) if t is not None]):
        raise ValueError("image_grad: tensors on different devices")
    if dres is not None and tuple(dres.shape) != (n, c0, h * sf, w * sf):
        raise ValueError(f"image_grad: dres {tuple(dres.shape)} != {(n, c0, h * sf, w * sf)}")
    hp = wp = ca = cina = cb = cinb = 0
    if ga is not None:
        if wa is None:
            raise ValueError("image_grad: ga without wa")
        _, hp, wp, ca = ga.shape
        if ga.shape[0] != n or tuple(wa.shape[::2]) != (ca, 3) or wa.shape[3] != 3 or wa.shape[1] < c0 or ca % 4:
            raise ValueError(f"image_grad: ga {tuple(ga.shape)} / wa {tuple(wa.shape)} do not match")
        cina = wa.shape[1]
    if gb is not None:
        if wb is None:
            raise ValueError("image_grad: gb without wb")
        cb = gb.shape[3]
        if tuple(gb.shape[:3]) != (n, h, w) or tuple(wb.shape[::2]) != (cb, 3) or wb.shape[3] != 3 or wb.shape[1] < c0 or cb % 4:
            raise ValueError(f"image_grad: gb {tuple(gb.shape)} / wb {tuple(wb.shape)} do not match {(n, h, w)}")
        cinb = wb.shape[1]
    if into is not None and tuple(into.shape) != (n, c0, h, w):
        raise ValueError(f"image_grad: into {tuple(into.shape)} != {(n, c0, h, w)}")
    out = into if into is not None else torch.empty((n, c0, h, w), dtype=torch.float32, device=dev)
    d = nat.ImageGradDesc(dres=nat.ptr(dres), ga=nat.ptr(ga), wa=nat.ptr(wa), gb=nat.ptr(gb), wb=nat.ptr(wb), dx=nat.ptr(out),
                          n=n, c0=c0, h=h, w=w, sf=sf, hp=hp, wp=wp, ca=ca, cina=cina, cb=cb, cinb=cinb, accumulate=int(into is not None))
    nat.check(nat.load().virnet_image_grad(C.byref(d), nat.stream_handle()), "image_grad")
    return out


def ca_gate(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor) -> Tensor:
    """CALayer gate [N,C] from NHWC features."""
    _dev_check(x, "x")
    n, h, w, c = x.shape
    cr = w1.shape[0]
    ts = [t.detach() for t in (w1, b1, w2, b2)]
    for t in ts:
        _dev_check(t, "CALayer parameter")
    gate = torch.empty((n, c), dtype=torch.float32, device=x.device)
    nat.check(nat.load().virnet_ca_gate(nat.ptr(x), *(nat.ptr(t) for t in ts), nat.ptr(gate), n, h, w, c, cr,
                                        nat.stream_handle()), "ca_gate")
    return gate


CA_FUSED_MAX_ITEMS = 16 * 1024      # float4 items of one image the fused CALayer kernel holds in a workgroup's registers


def ca_scale_add(hcv: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, skip: Tensor) -> Tensor:
    """RB_Layer tail (KNet.py:15-26,38): hcv * CALayer gate(hcv) + skip on NHWC tensors -- one launch for small maps (KernelNet's
    16 x 16 x 64), the gate + scale pair otherwise."""
    _dev_check(hcv, "hcv"); _dev_check(skip, "skip")
    n, h, w, c = hcv.shape
    if h * w * (c // 4) > CA_FUSED_MAX_ITEMS or c % 4 or 256 % c:
        return scale_add(hcv, ca_gate(hcv, w1, b1, w2, b2), skip)
    ts = [t.detach() for t in (w1, b1, w2, b2)]
    for t in ts:
        _dev_check(t, "CALayer parameter")
    out = torch.empty_like(hcv)
    nat.check(nat.load().virnet_ca_scale_add(nat.ptr(hcv), *(nat.ptr(t) for t in ts), nat.ptr(skip), nat.ptr(out), n, h, w, c, w1.shape[0],
                                             nat.stream_handle()), "ca_scale_add")
    return out


KNET_BODY_MAX = 16      # largest map side virnet_knet_body keeps on one CU


def knet_body(x: Tensor, layers) -> Tensor:
    """KernelNet's RB_Layers in ONE launch (csrc/knet_body.hip): ``x`` NHWC [n,h,w,64] with h, w <= 16; ``layers`` = one tuple
    (conv1 packing, conv2 packing, CALayer w1, b1, w2, b2) per RB_Layer, the packings carrying their split-fp16 image."""
    _dev_check(x, "x")
    n, h, w, c = x.shape
    arr = (nat.KnetLayer * len(layers))()
    keep = []
    for i, (p1, p2, w1, b1, w2, b2) in enumerate(layers):
        if p1.f16 is None or p2.f16 is None:
            raise RuntimeError("knet_body needs the split-fp16 weight images (VIRNET_CONV_FORM of the f16 family)")
        ts = [t.detach() for t in (w1, b1, w2, b2)]
        for t in ts:
            _dev_check(t, "CALayer parameter")
        keep.append(ts)
        arr[i] = nat.KnetLayer(nat.ptr(p1.f16), 0 if p1.bias is None else nat.ptr(p1.bias), nat.ptr(p2.f16), 0 if p2.bias is None else nat.ptr(p2.bias),
                               *(nat.ptr(t) for t in ts))
    out = torch.empty_like(x)
    cr = layers[0][2].shape[0]
    nat.check(nat.load().virnet_knet_body(nat.ptr(x), nat.ptr(out), arr, len(layers), n, h, w, c, cr, nat.stream_handle()),
              "knet_body")
    return out


def scale_add(hcv: Tensor, gate: Tensor, skip: Tensor) -> Tensor:
    """hcv * gate[n,c] + skip on NHWC tensors."""
    _dev_check(hcv, "hcv"); _dev_check(skip, "skip"); _dev_check(gate, "gate")
    n, h, w, c = hcv.shape
    out = torch.empty_like(hcv)
    nat.check(nat.load().virnet_scale_add(nat.ptr(hcv), nat.ptr(gate), nat.ptr(skip), nat.ptr(out), n, h * w, c,
                                          nat.stream_handle()), "scale_add")
    return out


def _sft_weights(att) -> Tuple[nat.SftWeights, list]:
    """The AttLayer's eight parameter pointers as the C struct -- cached in the layer's ParamCache and rebuilt when a parameter
    moved (the eager SISR forward built twelve of these per call: 527 `nn.Module.__getattr__` walks, tools/probes/host_profile_sisr.py)."""
    c1, c2, cm, ca = convs = [att._modules[k] for k in ("conv1", "conv2", "mul_conv", "add_conv")]      # (the dicts Module.__getattr__ would walk to)
    ps = [c._parameters[k] for c in convs for k in ("weight", "bias")]
    def build():
        ts = [p.detach() for p in ps]
        for t in ts:
            _dev_check(t, "AttLayer parameter")
        return nat.SftWeights(*(nat.ptr(t) for t in ts), e=c1.cin, nf1=c1.cout, nf2=c2.cout, nf=cm.cout), ts
    return att._cache.get(("sft",), ps, build)


def sft_vec(vec: Tensor, att) -> Tuple[Tensor, Tensor]:
    """AttLayer on spatially constant conditioning: (mul, add), each [N, nf]."""
    _dev_check(vec, "vec")
    n = vec.shape[0]
    wt, keep = _sft_weights(att)
    if vec.shape[1] != wt.e:
        raise ValueError(f"conditioning vector has {vec.shape[1]} channels, AttLayer expects {wt.e}")
    mul = torch.empty((n, wt.nf), dtype=torch.float32, device=vec.device)
    add = torch.empty_like(mul)
    nat.check(nat.load().virnet_sft_vec(nat.ptr(vec), C.byref(wt), nat.ptr(mul), nat.ptr(add), n, nat.stream_handle()),
              "sft_vec")
    return mul, add


SFT_MULTI_MAX = 16


def sft_vec_multi(vec: Tensor, atts) -> list:
    """``sft_vec`` for several AttLayers on the same vector in ONE launch per 16 layers (virnet_sft_vec_multi): [(mul, add), ...] in the
    order of ``atts``.  The SFT layers of a down path all depend on the conditioning vector alone; one launch instead of one per layer."""
    _dev_check(vec, "vec")
    n = vec.shape[0]
    out = []
    lib = nat.load()
    for i0 in range(0, len(atts), SFT_MULTI_MAX):
        group = atts[i0:i0 + SFT_MULTI_MAX]
        wts = (nat.SftWeights * len(group))()
        muls, adds = (C.c_void_p * len(group))(), (C.c_void_p * len(group))()
        keep = []
        for l, att in enumerate(group):
            wt, ts = _sft_weights(att)
            if vec.shape[1] != wt.e:
                raise ValueError(f"conditioning vector has {vec.shape[1]} channels, AttLayer expects {wt.e}")
            keep.append(ts)
            wts[l] = wt
            mul = torch.empty((n, wt.nf), dtype=torch.float32, device=vec.device)
            add = torch.empty_like(mul)
            muls[l], adds[l] = nat.ptr(mul), nat.ptr(add)
            out.append((mul, add))
        nat.check(lib.virnet_sft_vec_multi(nat.ptr(vec), wts, len(group), muls, adds, n, nat.stream_handle()), "sft_vec_multi")
    return out


def sft_apply(raw: Tensor, rec: Tensor, chan0: int, nchan: int, step: int, att) -> Tensor:
    """lrelu(raw * mul(e) + add(e)) with the AttLayer evaluated per pixel on channels [chan0, chan0+nchan) of ``rec``."""
    _dev_check(raw, "raw"); _dev_check(rec, "rec")
    n, h, w, nf = raw.shape
    wt, keep = _sft_weights(att)
    if nchan != wt.e or nf != wt.nf:
        raise ValueError(f"AttLayer({wt.e}->{wt.nf}) does not match conditioning {nchan} / features {nf}")
    if tuple(rec.shape) != (n, h * step, w * step, 16):
        raise ValueError(f"rec shape {tuple(rec.shape)} != {(n, h * step, w * step, 16)}")
    act = torch.empty_like(raw)
    nat.check(nat.load().virnet_sft_apply(nat.ptr(raw), nat.ptr(rec), C.byref(wt), nat.ptr(act), n, h, w, step, chan0,
                                          nat.stream_handle()), "sft_apply")
    return act


# ----------------------------------------------------------------------------------------------------------------------
# training step: weight / bias gradients and the layout helpers of the input-gradient convs
# ----------------------------------------------------------------------------------------------------------------------
def wgrad_route_rule(kind: str, stride: int, ks: int, f16_family: bool, bf16_form: bool, wgrad_f32: bool, oh: int, chi: int, cin: int, cout: int,
                     xt_bf16: Optional[bool] = None, yt_bf16: Optional[bool] = None) -> Tuple[str, bool]:
    """Which kernel a weight gradient runs on, from plain values: ``(route, bf16)`` -- route out of s1 | s2 | convt (the f16 pipe,
    csrc/wgrad_f16.hip: _WGRAD_MODES) | f32 (virnet_conv_wgrad); bf16 = the f16 pipe contracts bf16-rounded operands.  ``kind``: conv | convt;
    ``f16_family``, ``bf16_form``: the conv form; ``wgrad_f32``: VIRNET_WGRAD_FORM=f32; ``oh``: the LOW-resolution height (the row ring takes
    >= 5 rows); ``chi``: the stored channels of a stride-2 layer's high-resolution operand (the phase image takes whole 32-channel blocks);
    ``xt_bf16`` / ``yt_bf16``: the bf16 flag of each offered T image, None where none is offered.  bf16 form: the C->C layers contract
    bf16-rounded operands; a few-channel stride-1 layer (tail, head, conv_last, SNet conv1) stays fp32-class unless its big operand already
    exists as an emitted bf16 image -- then it takes that image instead of re-laying the tensor (its other operand is a 16-channel record).
    tests/test_wgrad_dispatch.py holds it to tests/golden/wgrad_calls.json."""
    f16 = f16_family and not wgrad_f32 and oh >= 5
    if kind == "convt":
        route = "convt" if f16 and chi % 32 == 0 else "f32"
    elif ks == 3 and stride == 1:
        route = "s1" if f16 else "f32"
    else:
        route = "s2" if ks == 3 and stride == 2 and f16 and chi % 32 == 0 else "f32"
    return route, route != "f32" and bf16_form and (min(cin, cout) >= 32 or (route == "s1" and bool(xt_bf16 or yt_bf16)))


def _wgrad_route(kind: str, stride: int, ks: int, oh: int, chi: int, cin: int = 32, cout: int = 32, xt=None, yt=None) -> Tuple[str, bool]:
    return wgrad_route_rule(kind, stride, ks, _f16_family(), conv_form() == "bf16", _env("VIRNET_WGRAD_FORM", "f16") == "f32", oh, chi, cin, cout,
                            None if xt is None else xt.bf16, None if yt is None else yt.bf16)


def conv_wgrad(x: Tensor, dy: Tensor, weight_shape: Tuple[int, ...], *, stride: int = 1, transposed: bool = False,
               in_slope: Optional[float] = None, in_mul: Optional[Tensor] = None, in_add: Optional[Tensor] = None,
               bias_channels: Optional[int] = None, xt: Optional[TImage] = None, yt: Optional[TImage] = None):
    """Weight gradient in the reference layout (OIHW, or IOHW 2x2 for the transposed conv) from NHWC forward input ``x`` and
    NHWC output gradient ``dy`` (for the transposed conv: the space-to-depth gradient).  With ``bias_channels`` the bias gradient
    (sum of ``dy`` over pixels, first ``bias_channels`` channels) is returned too -- ``(dw, db)`` -- fused into the f16 path's pass
    over ``dy`` where that path runs (wgrad_route_rule), a ``virnet_colsum`` launch otherwise.  ``xt`` / ``yt``: T images of the (staged)
    input / of ``dy`` that a convolution's epilogue already emitted (``conv_mfma(emit=...)``): the f16 path then skips its re-layout pass over
    that operand (``yt.db`` is the bias gradient)."""
    _dev_check(x, "x"); _dev_check(dy, "dy")
    n, h, w, cx = x.shape
    cy = dy.shape[3]
    if transposed:
        cin, cout, ks, route = weight_shape[0], weight_shape[1], 1, "f32"
    else:
        cout, cin, ks = weight_shape[0], weight_shape[1], weight_shape[2]
        route, bf = _wgrad_route("conv", stride, ks, h // stride, cx, cin, cout, xt, yt)
    if route != "f32":
        return _conv_wgrad_f16(route, x, dy, weight_shape, cin, cout, in_slope, in_mul, in_add, bf16=bf, bias_channels=bias_channels, xt=xt, yt=yt)
    dw = torch.zeros(weight_shape, dtype=torch.float32, device=x.device)
    rows = 4 * cout if transposed else cout
    ctr = torch.zeros(((rows + 31) // 32) * ((cin + 31) // 32), dtype=torch.int32, device=x.device)
    d = nat.WgradDesc(x=nat.ptr(x), dy=nat.ptr(dy), in_mul=nat.ptr(in_mul), in_add=nat.ptr(in_add), dw=nat.ptr(dw),
                      counters=nat.ptr(ctr), n=n, h=h, w=w,
                      cx=cx, cy=cy, cin=cin, cout=cout, ks=ks, stride=stride, transposed=int(transposed),
                      in_act=int(in_slope is not None), in_slope=0.0 if in_slope is None else in_slope)
    pix = n * (h // stride) * (w // stride)
    _timed_call(nat.load().virnet_conv_wgrad, (C.byref(d),), "conv_wgrad", ("wgrad", ks, stride, int(transposed)),
                2.0 * pix * cin * cout * (4 if transposed else ks * ks))
    if bias_channels is not None:
        return dw, colsum(dy, bias_channels)
    return dw


def conv_grads(conv, x: Tensor, dy: Tensor, *, stride: int = 1, in_slope: Optional[float] = None, in_mul: Optional[Tensor] = None,
               in_add: Optional[Tensor] = None, bias_channels=..., xt: Optional[TImage] = None, yt: Optional[TImage] = None):
    """``(dW, db or None)`` of a layer (networks.params.ConvParam; transposed: the 2x2 stride-2 one, ``dy`` its high-resolution gradient) --
    conv_wgrad / convt_wgrad under ONE return convention.  db is None for a layer without bias; ``bias_channels`` (default: the layer's
    cout) is for a ``dy`` that stores more channels than the layer has."""
    shape = tuple(conv.weight.shape)
    if conv.transposed:
        dw, db = convt_wgrad(x, dy, shape, xt=xt)
        return dw, (None if conv.bias is None else db)
    if conv.bias is None:
        return conv_wgrad(x, dy, shape, stride=stride, in_slope=in_slope, in_mul=in_mul, in_add=in_add, xt=xt, yt=yt), None
    return conv_wgrad(x, dy, shape, stride=stride, in_slope=in_slope, in_mul=in_mul, in_add=in_add,
                      bias_channels=conv.cout if bias_channels is ... else bias_channels, xt=xt, yt=yt)


def convt_dgrad(dy: Tensor, pw: PackedWeight) -> Tensor:
    """Input gradient [n,h,w,cin] of ConvTranspose2d(k=2, s=2) from the NHWC gradient of its output [n,2h,2w,cout] and the layer's
    dgrad packing: on the split-fp16 stride-2 kernel when the packing carries that form, else the fp32 pointwise GEMM over the
    space-to-depth gradient."""
    if pw.s2 is not None and pw.s2.f16 is not None and _f16_family():
        return conv_mfma(dy, pw.s2, stride=2, want_raw=True)[0]
    return conv_mfma(space_to_depth2(dy), pw, want_raw=True)[0]


def _wgrad_s2_ok(oh: int, chi: int) -> bool:
    """The stride-2 layers' weight gradients on the f16 pipe (wgrad_route_rule; the same conditions for the 3x3 stride-2 and the 2x2 transposed conv)"""
    return _wgrad_route("convt", 2, 2, oh, chi)[0] != "f32"


def convt_wgrad(x: Tensor, dy: Tensor, weight_shape: Tuple[int, ...], xt: Optional[TImage] = None):
    """(dw [cin][cout][2][2], db [cout]) of ConvTranspose2d(k=2, s=2) (UpBlock.upsampler, AttResUNet.py:80) from its NHWC input ``x``
    [n,h,w,cx] and the NHWC gradient of its output ``dy`` [n,2h,2w,cout]: on the f16 pipe (the bias gradient rides on the re-layout pass
    over ``dy``), or -- fp32 forms, tiny maps (wgrad_route_rule) -- the fp32 kernel on the space-to-depth gradient plus a column sum."""
    _dev_check(x, "x"); _dev_check(dy, "dy")
    n, h, w, cx = x.shape
    cin, cout = weight_shape[0], weight_shape[1]
    if tuple(dy.shape) != (n, 2 * h, 2 * w, cout):
        raise ValueError(f"dy shape {tuple(dy.shape)} != {(n, 2 * h, 2 * w, cout)}")
    route, bf = _wgrad_route("convt", 2, 2, h, cout, cin, cout)
    if route != "f32":
        return _conv_wgrad_f16(route, x, dy, weight_shape, cin, cout, None, None, None, bf16=bf, bias_channels=cout, xt=xt)
    return conv_wgrad(x, space_to_depth2(dy), weight_shape, transposed=True), colsum(dy)



def conv_wgrad_plan_query(n: int, h: int, w: int, cx: int, cy: int, mode: int = 0) -> dict:
    """What the f16-pipe weight gradient would plan for a shape, without launching and without a device
    (virnet_conv_wgrad_f16_plan_query): ``{kg, nwv, pairs, split, run, nxs, nsteps}``.  mode 0: stride-1 3x3, ``(h, w, cx, cy)`` the stored
    shapes of x and dy; 1: 3x3 stride-2 conv, 2: 2x2 transposed conv, ``(h, w)`` the LOW-resolution size and ``(cx, cy)`` the stored
    channels of the high- / low-resolution operand.  Raises with the library's message for a shape the launcher rejects."""
    out = nat.WgradF16Plan()
    nat.check(nat.load().virnet_conv_wgrad_f16_plan_query(n, h, w, cx, cy, mode, C.byref(out)), "conv_wgrad_f16_plan_query")
    return {k: getattr(out, k) for k, _ in nat.WgradF16Plan._fields_}


_WORKSPACES: dict = {}


def _workspace(tag: str, nbytes: int, device: torch.device) -> Tensor:
    """Grow-only scratch buffer per (device, stream, tag).  Launches on one stream are ordered, so consecutive users of the same
    buffer cannot overlap; going through the caching allocator for three ~200 MB blocks per weight gradient instead cost whole
    steps of hipMalloc stalls while its pools warmed up."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) if buf is not None else nbytes, dtype=torch.uint8, device=device)
        _WORKSPACES[key] = buf
    return buf


# The f16-pipe weight gradient (csrc/wgrad_f16.hip) per route of wgrad_route_rule: both operands are first re-laid channel-major as fp16
# hi/lo planes (T images), then contracted over pixels.  x always carries the forward conv's staging transform (in_slope / in_mul / in_add) and
# the layout pass over dy always yields the bias gradient; what differs per route is where the two sit:
#   a, b      the operands in the contraction's argument order ("x" | "dy"): a's image lives in workspace wgrad_xt, b's in wgrad_yt; b is the
#             LOW-resolution operand of a stride-2 layer, always in the plain layout (virnet_chsplit)
#   phase     a is the high-resolution operand of a stride-2 layer, laid out column-phase (virnet_chsplit_s2); else plain
#   offers    the operands an emitted T image is taken for
#   strict    an offered image of another geometry (or a released one) raises; else it is dropped and the tensor re-laid
#   fused_db  bias partials an offered image of dy still carries are reduced inside the contraction's own reduce launch
#             (virnet_conv_wgrad_f16_db, after which the image holds its db); else TImage.bias_sums() reduces them first
#   entry, scratch, mode   the contraction's entry point, its scratch sizer, the `mode` argument the entry point takes (None: it has none)
#   key, taps the timer key bench.py reads; flops = 2 * low-resolution pixels * cin * cout * taps
_WgradMode = namedtuple("_WgradMode", "a b phase offers strict fused_db entry scratch mode key taps")
_WGRAD_MODES = {
    "s1": _WgradMode("x", "dy", False, ("x", "dy"), True, True, "virnet_conv_wgrad_f16", "virnet_conv_wgrad_f16_scratch_bytes", None, ("wgrad_f16", 3, 1, 0), 9),
    "s2": _WgradMode("x", "dy", True, ("dy",), False, False, "virnet_conv_wgrad_f16_s2", "virnet_conv_wgrad_f16_s2_scratch_bytes", 0, ("wgrad_f16_s2", 3, 2, 0), 9),
    "convt": _WgradMode("dy", "x", True, ("x",), False, False, "virnet_conv_wgrad_f16_s2", "virnet_conv_wgrad_f16_s2_scratch_bytes", 1, ("wgrad_f16_s2", 2, 2, 1), 4),
}


def _wgrad_operand(t: Optional[TImage], what: str, geom: tuple, bf16: bool, nsums: Optional[int], strict: bool, tag: str, nbytes, device):
    """One operand of the f16-pipe weight gradient: ``(buffer, image)`` -- the offered T image ``t`` when it is THE image this call would build
    (geometry, operand form, and with ``nsums`` the channel sums of that many channels, reduced or pending), else ``(workspace, None)``: the
    tensor is to be laid out into the workspace, and that pass is where its channel sums come from."""
    if t is not None and ((t.n, t.h, t.w, t.c) != geom or t.buf is None):
        if strict:
            raise ValueError(f"conv_wgrad: {what} is a T image of {(t.n, t.h, t.w, t.c)}, expected {geom}")
        t = None
    if t is not None and t.bf16 != bf16:
        t = None                                            # (emitted by a conv of the other operand form: re-lay it)
    if t is not None and nsums is not None and not (t.db.numel() == nsums if t.db is not None else (t.col is not None and t.ncol == nsums)):
        t = None                                            # (no channel sums came with it: take the pass that produces them)
    return (t.buf, t) if t is not None else (_workspace(tag, nbytes(*geom), device), None)


def _conv_wgrad_f16(route: str, x: Tensor, dy: Tensor, weight_shape, cin: int, cout: int, in_slope, in_mul, in_add, *, bf16: bool,
                    bias_channels: Optional[int] = None, xt: Optional[TImage] = None, yt: Optional[TImage] = None):
    """Weight gradient on the f16 pipe, one straight line over the route's row of _WGRAD_MODES: take or lay out both operands, find the bias
    sums, contract.  ``dw`` or, with ``bias_channels``, ``(dw, db)``."""
    m, lib, st, dev, bc = _WGRAD_MODES[route], nat.load(), nat.stream_handle(), x.device, bias_channels
    ten, offered = {"x": x, "dy": dy}, {"x": (xt, "xt"), "dy": (yt, "yt")}
    n, oh, ow, cb = ten[m.b].shape
    ca = ten[m.a].shape[3]
    if m.phase and tuple(ten[m.a].shape[1:3]) != (2 * oh, 2 * ow):
        raise ValueError(f"stride-2 weight gradient: {tuple(ten[m.a].shape)} is not twice {tuple(ten[m.b].shape)}")
    ev = _timer_start()
    buf, img = {}, {}
    for nm, tag, nbytes in ((m.a, "wgrad_xt", lib.virnet_chsplit_s2_bytes if m.phase else lib.virnet_chsplit_bytes), (m.b, "wgrad_yt", lib.virnet_chsplit_bytes)):
        buf[nm], img[nm] = _wgrad_operand(offered[nm][0] if nm in m.offers else None, offered[nm][1], tuple(ten[nm].shape), bf16,
                                          bc if nm == "dy" else None, m.strict, tag, nbytes, dev)
    # ---- the bias sums: from the layout pass over dy (col: its per-block partials), or what the offered image of dy brought along
    db = col = None
    src = img["dy"] if bc is not None else None
    if bc is not None and src is None:
        db = _zeros(bc, dev)
        col = _workspace("wgrad_col", (lib.virnet_chsplit_s2_colsum_bytes if m.phase and m.a == "dy" else lib.virnet_chsplit_colsum_bytes)(*dy.shape), dev)
    elif src is not None and m.fused_db:
        db = src.db                                         # (None: partials the emitting conv left, reduced in OUR reduce launch below)
    elif src is not None:
        _zeros(bc, dev)                                     # (never used: keeps every later bias gradient of a zero_arena in the slice it always had)
        db = src.bias_sums()
    for nm, phase in ((m.a, m.phase), (m.b, False)):
        if img[nm] is None:
            pre = (int(in_slope is not None), 0.0 if in_slope is None else in_slope, nat.ptr(in_mul), nat.ptr(in_add)) if nm == "x" else (0, 0.0, None, None)
            sums = (nat.ptr(col), nat.ptr(db), bc) if nm == "dy" and col is not None else (None, None, 0)
            nat.check((lib.virnet_chsplit_s2 if phase else lib.virnet_chsplit)(nat.ptr(ten[nm]), *ten[nm].shape, *pre, int(bf16), nat.ptr(buf[nm]), *sums, st),
                      "chsplit_s2" if phase else "chsplit")
    dw = torch.empty(weight_shape, dtype=torch.float32, device=dev)                # every element is written by the reduction
    scr = _workspace("wgrad_part", getattr(lib, m.scratch)(n, oh, ow, ca, cb), dev)
    args = (nat.ptr(buf[m.a]), nat.ptr(buf[m.b]), nat.ptr(dw), nat.ptr(scr), n, oh, ow, ca, cb, cin, cout) + (() if m.mode is None else (m.mode,)) + (int(bf16),)
    if src is not None and db is None:
        src.col_fresh()
        db = _zeros(bc, dev)
        nat.check(lib.virnet_conv_wgrad_f16_db(*args, nat.ptr(src.col), nat.ptr(db), src.nblk, bc, st), "conv_wgrad_f16_db")
        src.db, src.col = db, None
    else:
        nat.check(getattr(lib, m.entry)(*args, st), m.entry[len("virnet_"):])
    if ev is not None:
        _timer_stop(ev, m.key, 2.0 * n * oh * ow * cin * cout * m.taps)
    return dw if bc is None else (dw, db)


def colsum(dy: Tensor, cvalid: Optional[int] = None) -> Tensor:
    """Bias gradient: sum of an NHWC tensor over pixels -> [cvalid]."""
    _dev_check(dy, "dy")
    c = dy.shape[-1]
    cvalid = c if cvalid is None else cvalid
    db = _zeros(cvalid, dy.device)
    nat.check(nat.load().virnet_colsum(nat.ptr(dy), nat.ptr(db), dy.numel() // c, c, cvalid, nat.stream_handle()), "colsum")
    return db


def sft_backward(da: Tensor, x: Tensor, mul: Tensor, add: Tensor, *, slope: float = 0.2, res: Optional[Tensor] = None):
    """Backward of ``a = leaky_relu(x*mul + add, slope)`` with per-image [N, C] vectors on NHWC tensors:
    ``(dx (+res), dmul, dadd)`` from ``da`` in one pass (csrc/small.hip::sft_backward_kernel)."""
    for t, nm in ((da, "da"), (x, "x"), (mul, "mul"), (add, "add")):
        _dev_check(t, nm)
    n, h, w, c = x.shape
    if tuple(da.shape) != (n, h, w, c) or tuple(mul.shape) != (n, c) or tuple(add.shape) != (n, c):
        raise ValueError(f"sft_backward: da {tuple(da.shape)} / mul {tuple(mul.shape)} / add {tuple(add.shape)} do not match x {tuple(x.shape)}")
    if res is not None:
        _dev_check(res, "res")
        if tuple(res.shape) != (n, h, w, c):
            raise ValueError(f"sft_backward: res {tuple(res.shape)} != {(n, h, w, c)}")
    lib = nat.load()
    dx = torch.empty_like(x)
    dmul = torch.empty((n, c), dtype=torch.float32, device=x.device)           # written, not accumulated onto: the sums are order-fixed
    dadd = torch.empty((n, c), dtype=torch.float32, device=x.device)
    nbytes = lib.virnet_sft_backward_scratch_bytes(n, h * w, c)
    if nbytes == 0:
        raise ValueError(f"sft_backward: unsupported shape {(n, h, w, c)} (c must be a multiple of 4, at most 1024)")
    part = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    nat.check(lib.virnet_sft_backward_ordered(nat.ptr(da), nat.ptr(x), nat.ptr(mul), nat.ptr(add), nat.ptr(res), slope, nat.ptr(dx), nat.ptr(dmul),
                                              nat.ptr(dadd), nat.ptr(part), n, h * w, c, nat.stream_handle()), "sft_backward_ordered")
    return dx, dmul, dadd


def zero_stuff2(dy: Tensor) -> Tensor:
    _dev_check(dy, "dy")
    n, h, w, c = dy.shape
    z = torch.empty((n, 2 * h, 2 * w, c), dtype=torch.float32, device=dy.device)
    nat.check(nat.load().virnet_zero_stuff2(nat.ptr(dy), nat.ptr(z), n, h, w, c, nat.stream_handle()), "zero_stuff2")
    return z


def space_to_depth2(dy: Tensor) -> Tensor:
    _dev_check(dy, "dy")
    n, h2, w2, c = dy.shape
    out = torch.empty((n, h2 // 2, w2 // 2, 4 * c), dtype=torch.float32, device=dy.device)
    nat.check(nat.load().virnet_space_to_depth2(nat.ptr(dy), nat.ptr(out), n, h2 // 2, w2 // 2, c, nat.stream_handle()), "space_to_depth2")
    return out


def pack_input_backward(drec: Tensor, chan: int, hw: Tuple[int, int], *, map_: Optional[Tensor] = None, map_sqrt: bool = False,
                        into: Optional[Tensor] = None) -> Tensor:
    """Gradient of one map channel of virnet_pack_input: [N,1,h,w] from the NHWC record gradient (reflect-pad adjoint, sqrt')."""
    _dev_check(drec, "drec")
    n, hp, wp, crec = drec.shape
    h, w = hw
    out = into if into is not None else torch.empty((n, 1, h, w), dtype=torch.float32, device=drec.device)
    nat.check(nat.load().virnet_pack_input_backward(nat.ptr(drec), crec, chan, nat.ptr(map_), nat.ptr(out), n, h, w, hp, wp,
                                                    int(map_sqrt), int(into is not None), nat.stream_handle()), "pack_input_backward")
    return out


# ---- inference-only conv forms ---------------------------------------------------------------------------------------------------
INFERENCE_ONLY_FORMS = ("wx4x1",)


def require_trainable_form(what: str) -> None:
    """Raises under an inference-only conv form: ``what`` names the operation that records for autograd, computes a gradient or asks a
    conv for a T image.  (wx4x1: single-product fp16 gradients underflow where bf16's do not -- that arithmetic has no numerics gate yet.)"""
    form = conv_form()
    if form in INFERENCE_ONLY_FORMS:
        raise RuntimeError(f"VIRNET_CONV_FORM={form} is an inference-only form: {what} needs a training form (wx4, f16x3, bf16, wino or direct); "
                           "run it under torch.no_grad() on a detached image, or pick another form")
