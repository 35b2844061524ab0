"""The bounds of forward_ref.py at the thin, odd and maximal tile shapes of forward_obs.SHAPE_TABLE (no GPU; method of
test_forward_ref_cpu.py: the oracle's own f16 / bf16 / fp32 forward plays the device).

At every (scale, shape, precision) that test_gpu_forward_shapes.py runs, the emulated correct forward must pass every group in the
single-layer and in the default-plan (hidden) form, with full coverage and no group refused by group_bound: the derived bounds are then
satisfiable by a correct kernel at maps of one row, one column and one pixel, and the GPU file needs no tolerance of its own.

The bounds are not vacuous there either: at 32 x 416 (stride-32 map 1 x 13: the top and the bottom halo are the same row) and 32 x 32
(1 x 1: one token, one pixel) a zeroed tap, a dropped bias, a swapped channel and a last-row mutation each fail the group they touch, at
the only row / the only pixel of the stride-32 map; so does a 3x3 kernel that reads the 1 x 13 map as 13 x 1."""
import functools

import numpy as np
import pytest

import forward_ref as fr
from forward_obs import SHAPE_TABLE
from test_forward_ref_cpu import PRECS, _fails, _hide, _model, _store

# what test_gpu_forward_shapes.py runs: n at the whole table plus the two tail=False batches, s at three shapes
SHAPES = {"n": tuple(SHAPE_TABLE) + ((32, 32, 5), (32, 416, 2)), "s": ((32, 32, 5), (32, 416, 2), (416, 32, 2))}
THIN = ((32, 416), (32, 32))  # stride-32 map 1 x 13 and 1 x 1


@functools.lru_cache(maxsize=4)
def _taps(scale, h, w, B, prec):
    m = _model(scale)
    x = np.random.default_rng(h + w + B).integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    taps = {}
    m.forward_raw(x, prec, taps)
    obs = {k: v for k, v in taps.items() if k in fr.graph(m)}
    obs["tile"] = x
    assert sum(n in obs for n in m.convs) == len(m.convs) == 96
    return m, obs


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("scale,h,w,B", [(s, h, w, B) for s in ("n", "s") for (h, w, B) in SHAPES[s]])
def test_correct_forward_satisfies_every_bound_at_thin_shapes(scale, h, w, B, prec):
    m, obs = _taps(scale, h, w, B, prec)
    assert obs["model.9.cv2"].shape[2:] == (h // 32, w // 32) and obs["model.0"].shape[0] == B
    everything = set(m.convs) | {"attn:model.10.m.0.attn", "up:up13", "up:up16"} | {f"pool:model.9.pool{i}" for i in range(3)}
    for form, o in (("single ", obs), ("fused ", _hide(m, obs))):
        ev = fr.Evaluator(m, prec, o)
        ratios, covered = fr.check_all(ev, [k for k in o if k != "tile"], label=f"{prec} {scale} {h}x{w} B{B} {form}")  # (a refused group asserts)
        assert covered == everything, everything ^ covered
        print(f"{prec} {scale} {h}x{w} B{B} {form}: worst ratio {max(ratios.values()):.3f} at {max(ratios, key=ratios.get)}")


# ---------------------------------------------------------------------------------------------- mutations on the stride-32 map
def _pixels(t):
    """the only pixel of a 1 x 1 map; the first and the middle pixel of the only row otherwise (that row is the first AND the last)"""
    H, W = t.shape[2:]
    assert H == 1
    return sorted({(0, 0), (0, W // 2)})


def _kernel_mutation(prec, h, w, name, hidden=False, **kw):
    """test_forward_ref_cpu._kernel_mutation at a thin shape: the group of `name` evaluated with a mutated kernel replaces the correct
    output at ONE pixel of the stride-32 map (all channels)"""
    m, obs = _taps("n", h, w, 2, prec)
    o = _hide(m, obs) if hidden else obs
    ref, E, _ = fr.group_bound(fr.Evaluator(m, prec, o), name)
    assert ref.shape[2:] == (1, w // 32)
    good = _store(ref, prec, name)
    fr.check_group(f"{prec} {h}x{w} {name} emulated, unmutated", good, ref, E)
    bad = _store(fr.Evaluator(m, prec, o, **kw).node(name)[0], prec, name)
    for (y, x) in _pixels(ref):
        got = good.clone()
        got[:, :, y, x] = bad[:, :, y, x]
        _fails(f"{prec} {h}x{w} {name} mutated at ({y}, {x})", got, ref, E)


def _centre_tap(w, b):
    w[:, :, 1, 1] = 0.0
    return w, b


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("h,w", THIN)
def test_zeroed_tap_fails_on_the_only_row(prec, h, w):
    """model.7: the stride-2 3x3 that makes the stride-32 map; the centre tap is the only one that never reads padding on a 1 x 1 map"""
    _kernel_mutation(prec, h, w, "model.7", mutate={"model.7": _centre_tap})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("h,w", THIN)
def test_zeroed_tap_in_a_hidden_layer_fails_on_the_only_row(prec, h, w):
    """inside the seven-conv C3k of the stride-32 map (c3kimg.hip hides its six inner layers)"""
    _kernel_mutation(prec, h, w, "model.8.m.0.cv3", hidden=True, mutate={"model.8.m.0.m.1.cv1": _centre_tap})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("h,w", THIN)
def test_dropped_bias_fails_on_the_only_row(prec, h, w):
    name = "model.9.cv1"
    c = int(_model("n").convs[name].b.abs().argmax())

    def drop(w_, b):
        b[c] = 0.0
        return w_, b
    _kernel_mutation(prec, h, w, name, mutate={name: drop})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("h,w", THIN)
def test_swapped_channels_fail_on_the_only_row(prec, h, w):
    """the two channels of the pixel that differ most (swapping two nearly equal values changes nothing a bound could see)"""
    m, obs = _taps("n", h, w, 2, prec)
    name = "model.10.cv2"
    ref, E, _ = fr.Evaluator(m, prec, obs).node(name)
    for (y, x) in _pixels(ref):
        c0, c1 = int(ref[0, :, y, x].argmax()), int(ref[0, :, y, x].argmin())
        got = obs[name].clone()
        got[0, [c0, c1], y, x] = got[0, [c1, c0], y, x]
        _fails(f"{prec} {h}x{w} {name} channels {c0} / {c1} swapped at ({y}, {x})", got, ref, E)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("h,w", THIN)
def test_last_row_mutation_fails_where_the_last_row_is_the_first(prec, h, w):
    """a halo row read as valid: the 3x3 of the stride-32 box branch sees the row above (= below) the only row as a copy of that row
    instead of zero padding -- the kernel rows 0 and 2 then add to row 1"""
    name = "model.23.cv2.2.0"

    def halo(w_, b):
        w_[:, :, 1] = w_[:, :, 0] + w_[:, :, 1] + w_[:, :, 2]
        return w_, b
    _kernel_mutation(prec, h, w, name, mutate={name: halo})


@pytest.mark.parametrize("prec", PRECS)
def test_1x13_map_read_as_13x1_fails(prec):
    """A planted H / W swap.  A 1 x 13 and a 13 x 1 map have the same NHWC bytes, so the swap shows in the neighbours a 3x3 conv reads: a
    kernel that takes the row of 13 for a column applies its taps (ky, kx) as (kx, ky) -- the transposed 3x3 weights on the true shape."""
    name = "model.23.cv2.2.0"

    def swap(w_, b):
        return w_.transpose(2, 3).contiguous(), b
    _kernel_mutation(prec, 32, 416, name, mutate={name: swap})
