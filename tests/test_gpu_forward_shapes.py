"""The inference path at thin, odd and maximal tile shapes (forward_obs.SHAPE_TABLE), per element against fp64 and device against device.

LetterBox(auto=True) pads a ragged border crop only to the next multiple of 32: a 10 x 416 crop of a 642 x 640 image IS a 32 x 416 network
input, and obb_forward accepts every multiple of 32 up to 1280.  Which kernel form runs is chosen from the map size in many places
(plan_conv, plan_conv32_nc, bneck_supported, dwpw_supported, stem_supported, c3k2f32_tile, upacc_ok, the SPPF form, conv_ni_supported), so
these shapes run forms and tile remainders that 416 x 416 and 128 x 128 never do: the width-keyed fused forms at the minimum height they
admit, a stride-32 map of one row (top and bottom halo are the same row) or one pixel (attention over one token, three 5x5 pools and the
depthwise `pe` on 1 x 1, upsample 1 -> 2), whole-image NI tiles whose last tile is partial, 1280-wide rows of several column tiles.

test_every_group_per_element_at_thin_shapes is forward_obs.check_every_group, the procedure of test_gpu_forward_elems.py unchanged, with the
bounds of forward_ref.py (test_forward_shapes_cpu.py shows that a correct forward satisfies them at exactly these shapes and that they still
catch a zeroed tap, a dropped bias, a swapped channel and an H / W swap on the one-row map).  The device-versus-device tests are bit for bit.

Plan forms of the default n plan at these shapes, read from the predicates and asserted in _assert_forms (every case prints its plan with -s):
  bneck   (bneck_supported: C 16 at W 104 / 32, C 32 at W 52 / 16, H % 4 == 0): 32 x 416 and 64 x 416 -- model.2 at 8 x 104 / 16 x 104,
          model.4 and model.16 at 4 x 52 / 8 x 52; nowhere else in the table (no other width is keyed)
  dwpw    (dwpw_supported: W 52 / 16 in 2- / 4-row stripes, W 26 / 8 in 2- / 8-row stripes): the four class-branch pairs of the stride-8 and
          stride-16 levels at 32 x 416 (4 x 52, 2 x 26) and 64 x 416
  stem    (stem_supported: Hin % 8 == 0, Win % 32 == 0, Win <= 416; fp32: stem32_supported, bounded by its LDS rows instead): every shape but
          32 x 1280; 1280 x 32 has Win = 32 and takes it
  front   (front_supported: both sides multiples of 52) and c3kimg (13 x 13 only): at no shape of the table
  NI      16-bit (conv_ni_supported: square 4 x 4 / 2 x 2 maps): 32 x 32 only; fp32 (plan_conv32_nc: a whole map within half a tile's
          pixels): the small maps of every shape"""
import re

import numpy as np
import pytest
import torch

from forward_obs import SHAPE_TABLE, check_every_group
from oracle.yolo11_obb import Yolo11OBB

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(scale, ch):
    if (scale, ch) not in _MODELS:
        _MODELS[scale, ch] = Yolo11OBB(scale, nc=12, ch=ch, seed=0)
    return _MODELS[scale, ch]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops as o
    yield o
    o.model_load(_model("n", 3).to_blob())


def _tiles(seed, B, h, w, ch=3):
    return torch.as_tensor(np.random.default_rng(seed).integers(0, 256, (B, h, w, ch), dtype=np.uint8)).cuda()


def _count(plan, start):
    return sum(l.startswith(start) for l in plan)


def _ni(plan):
    """the NI field of every conv / conv32 line"""
    return [int(v) for l in plan if l.startswith(("conv ", "conv32 ")) for v in re.findall(r" NI(\d+) ", l)]


def _assert_forms(plan, prec, h, w):
    """default plan of n, 3 channels: each fused form where its *_supported predicate admits the shape, and not where it does not"""
    assert _count(plan, "front ") == 0 and _count(plan, "c3kimg ") == 0, plan  # no side is a multiple of 52, no map is 13 x 13
    if prec == "f32":
        assert _count(plan, "stem32 ") == (0 if w > 416 else 1), plan
        assert sum(" upacc1 " in l for l in plan) == 2, plan  # upacc_ok: the stride-8 and stride-16 maps of a multiple of 32 are always even
        assert max(_ni(plan)) > 1, plan  # plan_conv32_nc: the small maps of every shape of the table, square or not
        return
    assert _count(plan, "stem ") == (0 if w > 416 else 1), plan
    keyed = w == 416  # stride-4 / -8 / -16 widths 104 / 52 / 26; h = 32, 64: heights 8 / 4 / 2 and 16 / 8 / 4, whole stripes
    assert sum(l.startswith("bneck ") and ".m.0+model." in l for l in plan) == (3 if keyed else 0), plan
    assert _count(plan, "dwpw ") == (4 if keyed else 0), plan
    assert (max(_ni(plan)) > 1) == ((h, w) == (32, 32)), plan  # conv_ni_supported: square 4 x 4 and 2 x 2 maps
    # plan_conv's stride-2 stripe form (64 input channels, Wout % 13 == 0, Hout >= 4: model.3 and model.17; model.5 has 128 input channels
    # and never takes it) on exactly ONE 4-row stripe: model.3 at 32 x 416, model.17 at 64 x 416; model.17 at 32 x 416 (2 x 26) declines
    stripe = lambda name, out: any(l.startswith(f"conv {name}") and f" {out} TH4 TW13 " in l for l in plan)
    if (h, w) == (32, 416):
        assert stripe("model.3+model.4.cv1 ", "out4x52") and not any(l.startswith("conv model.17 ") and " TH4 TW13 " in l for l in plan), plan
    if (h, w) == (64, 416):
        assert stripe("model.3+model.4.cv1 ", "out8x52") and stripe("model.17 ", "out4x26"), plan


CASES = [(p, True, "n", 3, h, w, B) for p in ("f32", "f16", "bf16") for (h, w, B) in SHAPE_TABLE] + \
        [(p, False, "n", 3, h, w, B) for p in ("f16", "bf16") for (h, w, B) in ((32, 32, 5), (32, 416, 2))] + \
        [(p, True, "s", 3, h, w, B) for p in ("f32", "f16") for (h, w, B) in ((32, 32, 5), (32, 416, 2), (416, 32, 2))] + \
        [(p, True, "n", 4, 32, 416, 2) for p in ("f32", "f16")]


@pytest.mark.parametrize("prec,tail,scale,ch,h,w,B", CASES, ids=lambda v: str(v))
def test_every_group_per_element_at_thin_shapes(ops, prec, tail, scale, ch, h, w, B):
    def plan_check(plan):
        print("\n".join(plan), flush=True)
        if tail and scale == "n" and ch == 3:
            _assert_forms(plan, prec, h, w)
    check_every_group(ops, _model(scale, ch), prec, tail, scale, ch, h, w, B, plan_check)


# ---------------------------------------------------------------------------------------------- device against device, bit for bit
def _same(a, b, what):
    assert torch.equal(a[..., :77].contiguous().view(torch.int32), b[..., :77].contiguous().view(torch.int32)), \
        (what, float((a - b)[..., :77].abs().max()))


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("h,w,B", [(32, 32, 70), (32, 416, 37)])
def test_a_tile_alone_equals_the_tile_inside_a_batch(ops, prec, h, w, B):
    """batch independence where tiles share a workgroup (NI whole-image tiles, resident workgroups walking tiles): first, last, middle, and
    the first and last member of the partial last NI tile"""
    ops.model_load(_model("n", 3).to_blob(), precision=prec)
    x = _tiles(50 + h + w, B, h, w)
    full = ops.forward(x).clone()
    for i in sorted({0, 1, B // 2, B - B % 16, B - 2, B - 1}):
        _same(ops.forward(x[i:i + 1].contiguous()), full[i:i + 1], f"{prec} {h}x{w} tile {i} of {B}")


PLAIN = dict(tail=False, upfold=False, sppf_fuse=False, stem=False)  # one generic kernel per layer (test_fp32_layer_taps)


@pytest.mark.parametrize("h,w,B", SHAPE_TABLE)
def test_fp32_default_plan_equals_one_kernel_per_layer(ops, h, w, B):
    """the claim of test_fp32_fused_forms_are_bit_identical (stem off on both sides: the row-stripe input layer sums in another order) at
    every shape of the table"""
    net = _model("n", 3)
    x = _tiles(60 + h + w, B, h, w)
    ops.model_load(net.to_blob(), precision="f32", **PLAIN)
    plan = ops.debug_plan(h, w)
    assert all(l.startswith(("conv32 ", "pw32 ", "dwconv ", "pool ", "upsample ", "attn ", "total_macs")) for l in plan), plan
    assert _count(plan, "conv32 ") + _count(plan, "pw32 ") == 96 - 7, plan
    plain = ops.forward(x).clone()
    ops.model_load(net.to_blob(), precision="f32", stem=False)
    fused = ops.debug_plan(h, w)
    assert len(fused) < len(plan) and any("|" in l for l in fused), fused  # merged sibling convs, fused tails: fewer launches
    _same(ops.forward(x), plain, f"f32 default vs plain {h}x{w}")


@pytest.mark.parametrize("h,w,B", [(32, 32, 70), (32, 416, 3), (416, 32, 3), (96, 96, 3)])
def test_fp32_single_switches_are_bit_identical(ops, h, w, B):
    """nc2 / blk32 / pw32 / upacc / xtile singly off against the default: each is a change of tiling, addresses or launch form that keeps
    every output's k order (test_gpu_fp32.py makes the claims at 416 / 128 / 64 x 96)"""
    net = _model("n", 3)
    x = _tiles(70 + h + w, B, h, w)
    ops.model_load(net.to_blob(), precision="f32")
    on = ops.forward(x).clone()
    for key in ("nc2", "blk32", "pw32", "upacc", "xtile"):
        ops.model_load(net.to_blob(), precision="f32", **{key: False})
        plan = ops.debug_plan(h, w)
        if key == "nc2":
            assert not any(" NC2 " in l for l in plan), plan
        if key == "pw32":
            assert _count(plan, "pw32 ") == 0, plan
        if key == "upacc":
            assert not any(" upacc1 " in l for l in plan), plan
        _same(ops.forward(x), on, f"f32 {key} off vs on {h}x{w}")


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("h,w,B", [(32, 32, 70), (64, 32, 37)])
def test_16bit_whole_image_tiles_are_bit_identical(ops, prec, h, w, B):
    """`nitile` on / off: 70 images of 4 x 4 / 2 x 2 maps are four full NI16 tiles and one of six; 64 x 32 has no square map and must
    plan (and compute) the same either way"""
    net = _model("n", 3)
    x = _tiles(80 + h + w, B, h, w)
    ops.model_load(net.to_blob(), precision=prec, nitile=False)
    assert max(_ni(ops.debug_plan(h, w))) == 1
    off = ops.forward(x).clone()
    ops.model_load(net.to_blob(), precision=prec)
    assert (max(_ni(ops.debug_plan(h, w))) > 1) == ((h, w) == (32, 32))
    _same(ops.forward(x), off, f"{prec} nitile on vs off {h}x{w}")
