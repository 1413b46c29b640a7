"""The launch rules of the split-fp16 convolution hosts (csrc/conv_plan.h) against a table recorded from the commit before they were a
function one can call: tests/golden/launch_plans.json (tests/golden/make_launch_plans.py says how it was recorded).  CPU only -- the query
(ops.conv_plan_query -> virnet_conv_plan_query) launches nothing, and every row gives the CU count it plans for."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from virnet_amd import _native, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("VIRNET_DETERMINISTIC", "VIRNET_WX4_MIN_WGS", "VIRNET_WX4_ROWS", "VIRNET_WX4_NREP", "VIRNET_WX4_WIDE", "VIRNET_WX4_PERSIST", "VIRNET_WX4_PERSIST_MIN",
         "VIRNET_F16_SPLIT_WGS", "VIRNET_F16_MREP", "VIRNET_S2_WIDE", "VIRNET_S2_SPLIT_TILES", "VIRNET_CONVT_KS", "VIRNET_CONVT_SLABS")
STATIC = ("VIRNET_S2_WIDE",)                 # read once per process: rows that set it run in a child process
LAUNCH = ("form", "rows", "ng", "nrep", "variant", "slab_base", "groups", "persistent")


def table():
    with open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")) as f:
        return json.load(f)["rows"]


def desc_of(row):
    """The descriptor of a table row: dummy non-NULL pointers by epilogue / pre-activation class (the recording driver's rule).
    kind 0: 3x3 NHWC, 1: transposed 2x2, 2: 3x3 planar store; epi 4 = two stored tensors, else residual | 2 * mask; pre 2 = SFT, 1 = LeakyReLU."""
    family, n, h, w, cin_pad, cout, stride, kind, epi, pre, emit, n_cu = row[:12]
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    d = _native.ConvDesc(x=p, wpack=p, bias=p, n=n, h=h, w=w, cin_pad=cin_pad, cout=cout, ks=1 if kind == 1 else 3, stride=stride,
                         epi=(_native.EPI_NHWC, _native.EPI_CONVT, _native.EPI_NCHW)[kind], n_pad=(cout, 4 * cout, 32)[kind], nrep=1,
                         slope=0.2, mask_slope=0.2)
    if epi == 4:
        d.y_raw = d.y_act = p
    else:
        if epi & 1:
            d.res = p
        if epi & 2:
            d.mask = p
        if kind == 2 or epi & 1:
            d.y_raw = p
        else:
            d.y_act = p
    if pre >= 1:
        d.in_act, d.in_slope = 1, 0.2
    if pre == 2:
        d.in_mul = d.in_add = p
    if kind == 2:
        d.crop_h, d.crop_w = h, w
    d._keep = buf
    return d


def query(row):
    """the launches as the table writes them, or the library's error text"""
    try:
        return [[l[k] for k in LAUNCH] for l in ops.conv_plan_query(row[0], desc_of(row), emit_rows=row[10], n_cu=row[11])]
    except RuntimeError as e:
        return str(e).split("conv_plan_query: ", 1)[1]


def check_rows(rows, setenv, delenv):
    bad = []
    for row in rows:
        for k in KNOBS:
            delenv(k)
        for k, v in row[12].items():
            if k not in STATIC:
                setenv(k, v)
        got = query(row)
        if got != row[13]:
            bad.append((row[:13], row[13], got))
    return bad


def test_table_covers_every_host_and_knob():
    rows = table()
    assert 300 <= len(rows)
    assert {r[0] for r in rows} == {0, 1, 2, 3} and {r[7] for r in rows} == {0, 1, 2} and {r[6] for r in rows} == {1, 2}
    assert {r[11] for r in rows} == {256, 304, 64} and {r[10] for r in rows} == {0, 8, 16}
    forms = {l[0] for r in rows if isinstance(r[13], list) for l in r[13]}
    assert forms == {0, 1, 2, 3, 4, 5}                                # every kernel family is taken somewhere, the persistent one included
    assert any(isinstance(r[13], str) for r in rows)                  # rejected descriptors are rows too
    assert {k for r in rows for k in r[12]} == set(KNOBS)


def test_query_returns_the_recorded_launches(monkeypatch):
    rows = [r for r in table() if not any(k in r[12] for k in STATIC)]
    monkeypatch.delenv("VIRNET_S2_WIDE", raising=False)               # (a static: this process must not have started with it)
    bad = check_rows(rows, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ, first: {bad[:3]}"


def test_per_process_knob_in_a_child_process():
    """VIRNET_S2_WIDE is read once per process: its rows run in a child that starts with it set."""
    rows = [r for r in table() if "VIRNET_S2_WIDE" in r[12]]
    assert rows and all(r[12]["VIRNET_S2_WIDE"] == "0" for r in rows)
    code = ("import os, sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_launch_plan as t\n"
            "rows = [r for r in t.table() if 'VIRNET_S2_WIDE' in r[12]]\n"
            "bad = t.check_rows(rows, os.environ.__setitem__, lambda k: k in t.STATIC or os.environ.pop(k, None))\n"
            "print(json.dumps([len(rows), bad]))") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, VIRNET_S2_WIDE="0", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    n, bad = json.loads(out.stdout.strip().splitlines()[-1])
    assert n == len(rows) and not bad, bad[:3]


def test_query_rejects_bad_arguments():
    lib = _native.load()
    d = desc_of([1, 1, 64, 64, 96, 96, 1, 0, 0, 0, 0, 256])
    out = (_native.ConvLaunch * 4)()
    assert lib.virnet_conv_plan_query(7, ctypes.byref(d), 0, 256, out, 4) < 0 and b"bad family" in lib.virnet_last_error()
    assert lib.virnet_conv_plan_query(1, ctypes.byref(d), 16, 256, out, 4) < 0 and b"emit_rows" in lib.virnet_last_error()
    assert lib.virnet_conv_plan_query(1, None, 0, 256, out, 4) < 0 and b"desc is NULL" in lib.virnet_last_error()
    # cap smaller than the plan: the count is still the plan's, only `cap` records are written
    d = desc_of([1, 32, 64, 64, 96, 160, 1, 0, 0, 0, 0, 256])
    out[1].form = -7
    assert lib.virnet_conv_plan_query(1, ctypes.byref(d), 0, 256, out, 1) == 2 and out[1].form == -7
    with pytest.raises(RuntimeError, match="cout=80 must be a multiple of 32"):
        ops.conv_plan_query(_native.PLAN_WX4, desc_of([0, 1, 64, 64, 96, 80, 1, 0, 0, 0, 0, 256]), n_cu=256)
