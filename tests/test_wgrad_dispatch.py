"""The host side of the weight gradients -- ops.wgrad_route_rule and the conv_wgrad / convt_wgrad built on it -- against a call trace
recorded from the commit before the rule existed: tests/golden/wgrad_calls.json (tests/golden/make_wgrad_calls.py says how it was recorded,
and from what).  CPU only: the calls run on CPU tensors with every launch replaced by a logger; the rule takes plain values."""
import importlib.util
import json
import os

import wgrad_cases as wc
from virnet_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
spec = importlib.util.spec_from_file_location("make_wgrad_calls", os.path.join(GOLDEN, "make_wgrad_calls.py"))
rec = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rec)


def table():
    with open(os.path.join(GOLDEN, "wgrad_calls.json")) as f:
        tab = json.load(f)
    assert tab["envs"] == rec.ENVS and tab["recorded_from"]
    return [(tuple(c[:4]), dict(rec.EMPTY, **tab["traces"][c[4]])) for c in tab["cases"]]


def test_table_is_the_whole_grid_and_shows_every_route_and_bias_source():
    tab = table()
    assert [c for c, _ in tab] == rec.cases()
    assert {c[0] for c, _ in tab} >= {r.id for r in wc.ROWS} | set(rec.FALLBACK)
    assert {rec.route_of(t) for _, t in tab} >= set(rec.ROUTES)
    assert {rec.bias_source_of(t) for _, t in tab} >= set(rec.BIAS_SOURCES)
    for sid in rec.FALLBACK:                                # the fallback shapes never reach the f16 pipe
        assert {rec.route_of(t) for c, t in tab if c[0] == sid} == {"f32"}, sid
    wrong = [t for c, t in tab if c[2] == "wronggeom"]
    assert any(t["exc"] and t["exc"][0] == "ValueError" for t in wrong) and any(t["exc"] is None and rec.route_of(t) in ("s2", "convt") for t in wrong)


def test_calls_reproduce_the_recorded_traces():
    tab = table()
    with rec.Driver(ops) as run:
        bad = [(case, got, want) for case, want in tab for got in [json.loads(json.dumps(run(case)))] if got != want]
    assert not bad, f"{len(bad)} of {len(tab)} traces differ, first: {bad[:2]}"


def test_rule_reproduces_the_recorded_routes():
    """wgrad_route_rule from plain values alone against what the parent launched: the route, and the bf16 flag of the contraction"""
    bad = []
    for (sid, bias, offer, env), t in table():
        if t["exc"] is not None:
            continue
        mode, ks, cin, cout, cx, cy, n, h, w, _, _ = rec.SHAPES[sid]
        form = rec.ENVS[env].get("VIRNET_CONV_FORM", ops.DEFAULT_CONV_FORM)
        flag = (form == "bf16" and min(cin, cout) >= 32) != (offer == "otherform")      # make_wgrad_calls.Driver.run: the offered images' form
        got = ops.wgrad_route_rule("convt" if mode == wc.CONVT else "conv", 1 if mode == wc.S1 else 2, ks, form in ops._F16_FAMILY, form == "bf16",
                                   rec.ENVS[env].get("VIRNET_WGRAD_FORM") == "f32", h, cy if mode == wc.CONVT else cx, cin, cout,
                                   flag if "xt" in t["images"] else None, flag if "yt" in t["images"] else None)
        want = (rec.route_of(t), bool(rec.contraction_bf16(t)))
        if got != want:
            bad.append(((sid, bias, offer, env), got, want))
    assert not bad, f"{len(bad)} routes differ, first: {bad[:3]}"


def test_wgrad_s2_ok_is_the_rule(monkeypatch):
    for k in rec.KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert ops._wgrad_s2_ok(5, 32) and not ops._wgrad_s2_ok(4, 32) and not ops._wgrad_s2_ok(5, 40)
    monkeypatch.setenv("VIRNET_WGRAD_FORM", "f32")
    assert not ops._wgrad_s2_ok(24, 96)
    monkeypatch.delenv("VIRNET_WGRAD_FORM")
    monkeypatch.setenv("VIRNET_CONV_FORM", "wino")
    assert not ops._wgrad_s2_ok(24, 96)
