"""ops.pack_images_rule -- which images a packing carries -- and the pack_weight built on it, against a table recorded from the commit
before the rule existed: tests/golden/pack_images.json (tests/golden/make_pack_images.py says how it was recorded, and from what).
CPU only: the rule takes plain values and reads the conv form; pack_weight runs on `meta` tensors with the device calls cut out."""
import importlib.util
import json
import os

from virnet_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _script("make_pack_images")


def table():
    with open(os.path.join(GOLDEN, "pack_images.json")) as f:
        tab = json.load(f)
    assert tab["envs"] == rec.ENVS and tab["fields"] == list(rec.FIELDS)
    return [(tuple(r[:5]), env, p) for r in tab["rows"] for env, p in zip(tab["envs"], r[5], strict=True)]


def _present(p):
    return set(p["images"]) | ({"s2"} if "s2" in p else set())


def test_table_is_the_whole_grid_and_shows_every_image_both_ways():
    tab = table()
    fwd = [row for row, env, _ in tab if env == {} and not row[0].endswith("_dgrad")]
    assert fwd == rec.FORWARD and len(tab) == 58 * len(rec.ENVS)
    dgrad = {row for row, _, _ in tab if row[0].endswith("_dgrad")}
    assert dgrad == {(k + "_dgrad", s, ks, ci, co) for k, s, ks, ci, co in rec.FORWARD if ks != 1}      # every 3x3 and 2x2 layer has one
    for kind, names in rec.CARRIES.items():
        got = [_present(p) for row, _, p in tab if row[0] == kind]
        for name in names:
            assert any(name in g for g in got) and any(name not in g for g in got), (kind, name)


def test_rule_reproduces_the_recorded_image_sets(monkeypatch):
    bad = []
    for row, env, p in table():
        for k in rec.KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        names = ops.pack_images_rule(*row)
        fields = [ops._IMAGE_PACKERS[n][0] for n in names]
        with ops.forward_scope():
            scoped = ops.pack_images_rule(*row)
        if set(fields) != _present(p) or len(set(fields)) != len(fields) or scoped != names or ("f16_convt" in names) != (row[0] == "convt" and "f16" in p["images"]):
            bad.append((row, env, names, sorted(_present(p))))
    assert not bad, f"{len(bad)} rows differ, first: {bad[:3]}"


def test_pack_weight_reproduces_sets_sizes_and_fields():
    tab = table()
    with rec.Driver(ops) as run:
        bad = [(row, env, got, p) for row, env, p in tab for got in [run(row, env)] if got != p]
    assert not bad, f"{len(bad)} of {len(tab)} packings differ, first: {bad[:2]}"


def test_pack_weight_keeps_its_errors():
    import pytest
    import torch
    w = lambda *shape: torch.empty(shape, device="meta")
    with rec.Driver(ops):
        with pytest.raises(ValueError, match="dgrad packing handles 3x3 convs and the 2x2 transposed conv"):
            ops.pack_weight(w(8, 4, 1, 1), None, dgrad=True)
        with pytest.raises(ValueError, match=r"only ConvTranspose2d\(k=2, s=2\) is on the path"):
            ops.pack_weight(w(8, 4, 3, 3), None, transposed=True)
        with pytest.raises(ValueError, match="unsupported kernel 5x5"):
            ops.pack_weight(w(8, 4, 5, 5), None)
        with pytest.raises(ValueError, match="unsupported kernel 3x1"):
            ops.pack_weight(w(8, 4, 3, 1), None)


# pack_images.json row -> the layer of tests/golden/conv_forms.json that launches it (make_conv_forms.LAYERS), where that table has one
def _conv_forms_layer(row):
    kind, stride, ks, cin, cout = row
    if kind in ("conv", "conv_dgrad") and (stride, ks) == (1, 3) and cin == cout and cin >= 64:
        return "cc%d" % cin                                    # (the input gradient of a C->C layer is a C->C layer)
    return {("conv", 1, 3, 16, 96): "entry", ("conv", 1, 3, 96, 3): "exit", ("conv", 1, 3, 96, 4): "thin_dgrad", ("conv", 2, 3, 96, 192): "s2",
            ("convt", 2, 2, 192, 96): "convt", ("convt_dgrad", 2, 2, 192, 96): "convt_dgrad"}.get(row)


def test_image_sets_are_ones_the_launch_table_was_recorded_with(monkeypatch):
    """The two golden tables must not drift apart: every image set packing produces for a layer that conv_forms.json knows is one of the
    sets that table tried the layer with, and conv_form_rule, given the set as its has_* inputs, picks a form whose image the set has."""
    layers = _script("make_conv_forms").LAYERS
    seen = set()
    for row, env, p in table():
        name = _conv_forms_layer(row)
        if name is None:
            continue
        seen.add(name)
        transposed, stride, c, cout, cstore, _, sets = layers[name]
        have = set((p.get("s2", {"images": {}}) if name == "convt_dgrad" else p)["images"]) & {"wino", "f16", "bf16", "wx4"}
        assert "+".join(k for k in ("wino", "f16", "bf16", "wx4") if k in have) in sets, (row, env, have, sets)
        for k in rec.KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for n, h, w in ((1, 16, 16), (32, 128, 128)):
            form, _ = ops.conv_form_rule("wino" in have, "f16" in have, "bf16" in have, "wx4" in have, bool(transposed), stride, cstore == cout,
                                         n, h, w, c, cout, False, False, False, False, True, False, False)
            assert form == "direct" or ops._CONV_FORMS[form][1] in have, (row, env, have, form)
    assert seen == set(layers)
