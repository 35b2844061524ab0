"""The per-element bounds of forward_ref.py are satisfiable and not vacuous (no GPU).

The oracle's own "f16" / "bf16" forward with taps (torch on the CPU: the same rounding model, another summation order) plays the device, its
"fp32" forward plays the fp32 path.  Every group -- the single-layer groups, and the multi-layer groups left when the intermediates the
default plan hides are hidden -- must pass with no element excluded; every mutation of the emulated output or of the emulated kernel must
make check_group fail for the group it touches, at a border pixel and at an interior pixel."""
import functools

import numpy as np
import pytest
import torch

import forward_ref as fr
from oracle.yolo11_obb import Yolo11OBB, half_round

PRECS = ["f16", "bf16", "fp32"]


@functools.lru_cache(maxsize=None)
def _model(scale):
    return Yolo11OBB(scale, nc=12, ch=3, seed=0)


@functools.lru_cache(maxsize=None)
def _taps(scale, h, w, prec):
    m = _model(scale)
    x = np.random.default_rng(h + w).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    taps = {}
    head = m.forward_raw(x, prec, taps)
    obs = {k: v for k, v in taps.items() if k in fr.graph(m)}
    obs["tile"] = x
    assert sum(n in obs for n in m.convs) == len(m.convs) == 96
    return m, obs, head


def _hide(m, obs):
    hid = fr.hidden_in_default_plan(m)
    out = {k: v for k, v in obs.items() if k not in hid}
    out["model.10.a"] = obs["model.10.cv1"][:, :m.psa_c]
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("scale,h,w", [("n", 128, 128), ("n", 64, 96), ("s", 64, 64)])
def test_correct_forward_satisfies_every_bound(scale, h, w, prec):
    m, obs, _ = _taps(scale, h, w, prec)
    everything = set(m.convs) | {"attn:model.10.m.0.attn", "up:up13", "up:up16"} | {f"pool:model.9.pool{i}" for i in range(3)}
    for form, o in (("single ", obs), ("fused ", _hide(m, obs))):
        ev = fr.Evaluator(m, prec, o)
        ratios, covered = fr.check_all(ev, [k for k in o if k != "tile"], label=f"{prec} {scale} {h}x{w} {form}")
        assert covered == everything, everything ^ covered
        print(f"{prec} {scale} {h}x{w} {form}: worst ratio {max(ratios.values()):.3f} at {max(ratios, key=ratios.get)}")
    # the fused form really has multi-layer groups: model.2.cv1 reaches back to the tile, the stride-32 C3k is seven convs
    ev = fr.Evaluator(m, prec, _hide(m, obs))
    assert ev.node("model.2.cv1")[2] == {"model.0", "model.1", "model.2.cv1"}
    assert len(ev.node("model.8.m.0.cv3")[2]) == (7 if scale == "n" else 1)


# ---------------------------------------------------------------------------------------------- mutations
def _ulp16(v, prec):
    return 2.0 ** (torch.floor(torch.log2(v.abs())) - (10 if prec == "f16" else 7))


def _store(v, prec, name):
    """fp64 value -> what a correct device would store (fp32 for the fp32 path and the head columns)"""
    v = v.float()
    return v if prec == "fp32" or fr.is_head(name) else half_round(v, prec)


def _pixels(t, last_row=False):
    H, W = t.shape[2:]
    return [(H - 1, 0), (H - 1, W // 2)] if last_row else [(0, 0), (H // 2, W // 2)]


def _fails(what, got, ref, E):
    with pytest.raises(AssertionError):
        fr.check_group(what, got, ref, E)


def _kernel_mutation(prec, name, hidden, last_row=False, **kw):
    """The group of `name` with a mutated kernel (Evaluator hooks) plays the device; its output replaces the correct one at ONE pixel
    (all channels).  `hidden`: evaluate the fused form (the mutation sits in a hidden layer)."""
    m, obs, _ = _taps("n", 64, 96, prec)
    o = _hide(m, obs) if hidden else obs
    ref, E, _ = fr.group_bound(fr.Evaluator(m, prec, o), name)
    good = _store(ref, prec, name)
    fr.check_group(f"{prec} {name} emulated, unmutated", good, ref, E)
    bad = _store(fr.Evaluator(m, prec, o, **kw).node(name)[0], prec, name)
    for (y, x) in _pixels(ref, last_row):
        got = good.clone()
        got[:, :, y, x] = bad[:, :, y, x]
        _fails(f"{prec} {name} mutated at ({y}, {x})", got, ref, E)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_two_units_in_the_last_place_fail(prec):
    m, obs, _ = _taps("n", 64, 96, prec)
    name = "model.2.cv1"
    ref, E, _ = fr.Evaluator(m, prec, obs).node(name)
    for (y, x) in _pixels(ref):
        c = int(ref[0, :, y, x].abs().argmax())
        got = obs[name].clone()
        got[0, c, y, x] += 2 * _ulp16(got[0, c, y, x], prec)
        _fails(f"{prec} {name} + 2 ulp at ({y}, {x})", got, ref, E)


@pytest.mark.parametrize("prec", PRECS)
def test_dropped_bias_fails(prec):
    m = _model("n")
    name = "model.4.cv1"
    c = int(m.convs[name].b.abs().argmax())

    def drop(w, b):
        b[c] = 0.0
        return w, b
    _kernel_mutation(prec, name, False, mutate={name: drop})


@pytest.mark.parametrize("prec", PRECS)
def test_tap_zeroed_on_the_last_row_fails(prec):
    name = "model.17"

    def tap(w, b):
        w[:, :, 1, 1] = 0.0
        return w, b
    _kernel_mutation(prec, name, False, last_row=True, mutate={name: tap})


@pytest.mark.parametrize("prec", PRECS)
def test_swapped_channels_fail(prec):
    m, obs, _ = _taps("n", 64, 96, prec)
    name = "model.13.cv2"
    ref, E, _ = fr.Evaluator(m, prec, obs).node(name)
    for (y, x) in _pixels(ref):
        got = obs[name].clone()
        got[0, [0, 1], y, x] = got[0, [1, 0], y, x]
        _fails(f"{prec} {name} channels 0 / 1 swapped at ({y}, {x})", got, ref, E)


@pytest.mark.parametrize("prec", PRECS)
def test_silu_with_1e3_relative_error_fails(prec):
    _kernel_mutation(prec, "model.9.cv1", False, silu_fn=lambda z: fr.silu(z) * (1.0 + 1e-3))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,hid", [("model.2.cv2", "model.2.m.0.cv1"), ("model.2.cv1", "model.0"), ("model.23.cv3.0.2", "model.23.cv3.0.1.0"),
                                      ("model.8.m.0.cv3", "model.8.m.0.m.1.cv1"), ("model.22.m.0.cv3", "model.22.m.0.m.0.cv2")])
def test_tap_zeroed_in_a_hidden_layer_fails(prec, name, hid):
    def tap(w, b):
        w[:, :, 1, 1] = 0.0
        return w, b
    _kernel_mutation(prec, name, True, mutate={hid: tap})


def test_fp32_element_moved_by_1e5_fails():
    m, obs, _ = _taps("n", 64, 96, "fp32")
    name = "model.23.cv3.0.0.0"
    ref, E, _ = fr.Evaluator(m, "fp32", obs).node(name)
    for (y, x) in _pixels(ref):
        got = obs[name].clone()
        got[0, 3, y, x] += 1e-5 * max(abs(float(ref[0, 3, y, x])), 1.0)
        _fails(f"fp32 {name} + 1e-5 at ({y}, {x})", got, ref, E)
