"""The forward per element against fp64 away from the one point the rest of the suite sits on (YOLO11n, nc = 12): YOLO11s in fp32, and
class counts whose head slices are unaligned or partial.  Method, reference and bound are those of test_gpu_forward_elems.py
(forward_ref.py: |got - fp64| <= E for EVERY element of every group, E derived, no tolerance of this file's own).

Why these points.  Every support predicate of the engine keys on channel counts.  At s every count doubles: model.9.cv2 (cin 1024 > 512)
leaves k_pw_f32 for k_conv_f32, the 512-input 1x1s take the 16-wave k_pw_f32 form, C2PSA has 4 heads and a longer qkv permutation,
c3k2f32 (C == 16) drops out, stem32 runs at cout 32, the class branch is 128 wide.  The head row is [64 box | nc class | 1 angle] padded
to a multiple of 4 floats; only with nc % 4 == 0 does every slice start on a float4 and the class slice consist of whole float4s:
  nc  1  class slice one float, angle at column 65
  nc 13  angle at 77 (unaligned), class slice 3 float4s + 1
  nc 15  class slice partial, 65 + nc == 80 == padded width: no padding column at all
  nc 16  the fused-tail boundary of dwpw (tail_cout <= 16, % 4 == 0), angle at 80
  nc 20  aligned, but beyond that boundary
  nc 80  class-branch width c3 = max(64, min(nc, 100)) = 80: leaves pw32 (cout % 64) and the fused tail (cout2 <= 64)
A class store rounded up to a whole float4 lands in the angle column, an angle store rounded down lands in the last class: both are
checked because EVERY column [0, 65 + nc) of every anchor of every level is inside a checked group (forward_obs._head_obs).  The padding
columns [65 + nc, padded) are unspecified and not asserted.

Every per-element case: one forward into a guarded head buffer, every observable tensor read back, every group checked, the coverage
assertions of test_every_group_per_element (96 conv records, attention core, 3 pools, 2 upsample + concat reads, 9 head convs), then a
replay on a side stream: head bit for bit, guards intact, worst group again.  Plan-form assertions are pinned to what debug_plan printed
for these models on an MI355X.

Device against device (s, fp32): DESIGN section 3.0 claims bit-identity for the fused forms of the default plan against one kernel per
layer (with `stem` off on both sides: the row-stripe input layer sums its 27 taps in another order), and for nc2 / blk32 / pw32 / upacc /
xtile singly against the default.  `c3k2f` has nothing to switch at s (c3k2f32 needs C == 16; model.2's Bottleneck has 32 channels at s):
the plans must be EQUAL, which is what its case asserts.

Measured (worst |err| / bound per family, MI355X, 40 cases; records, not thresholds -- the thresholds are the derived bounds):
  s per layer, f32     single-layer groups 0.418 (model.10.m.0.attn.pe, 416x416); with the upsample + concat read 0.017 (model.16.cv1)
  s default, f32       single-layer groups 0.398 (model.10.m.0.attn.pe, 416x416); multi-layer 0.031 (DW -> model.23.cv3.0.0.1, 128x160)
  nc variants, f32     single-layer groups 0.339 (model.10.m.0.attn.pe, 64x96, every nc); multi-layer 0.040 (DW -> model.23.cv3.0.0.1, nc 13, 416x416)
  nc variants, f16     single-layer groups 0.995 (model.23.cv3.0.1.0, nc 13 / 20, 416x416); multi-layer 0.866 (model.6.m.0.m.0.cv2, nc 13, 416x416)
  nc variants, bf16    single-layer groups 0.995 (model.23.cv3.2.0.0, nc 16 / 80, 416x416); multi-layer 0.976 (upsample + concat -> model.16.cv1, nc 13, 64x96)
As in test_gpu_forward_elems.py the 16-bit single-layer groups sit just below 1 because round-to-nearest attains the store term.

Found by this file: with `stem=False` (and wherever stem32 does not take the input layer) the generic fp32 kernel was planned with two cout
fragments per workgroup for the 32 output channels of the s input layer, a form the uint8 input path is not built in: the forward
failed with "launch of 'model.0' failed: invalid argument".  plan_conv32 now keeps the uint8 layer at one fragment (two cout blocks);
test_s_fp32_every_layer_on_its_own and test_s_fp32_forms_are_bit_identical are its regression tests.
"""
import numpy as np
import pytest
import torch

import bounds
import forward_ref as fr
from forward_obs import _head_obs, _observe, _read, _stale, head_width, head_width_padded
from oracle.yolo11_obb import Yolo11OBB

pytestmark = pytest.mark.gpu

PER_LAYER = dict(tail=False, upfold=False, sppf_fuse=False, stem=False)  # one generic kernel per layer: every activation exists
_MODELS = {}


def _model(scale, nc, ch):
    if (scale, nc, ch) not in _MODELS:
        _MODELS[scale, nc, ch] = Yolo11OBB(scale, nc=nc, ch=ch, seed=0)
    return _MODELS[scale, nc, ch]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops as o
    yield o
    o.model_load(_model("n", 12, 3).to_blob())


def _tiles(seed, B, h, w, ch):
    return np.random.default_rng(seed).integers(0, 256, (B, h, w, ch), dtype=np.uint8)


def _count(plan, *needles, start=None):
    return sum(all(n in l for n in needles) and (start is None or l.startswith(start)) for l in plan)


def _fused_tails(plan):
    """conv32 lines that carry a trailing 1x1 (` tailN `, N = its cout)"""
    return [l for l in plan if l.startswith("conv32 ") and " tail" in l and " tail0 " not in l]


def _per_element(ops, m, prec, kw, h, w, B, label, plan_check=None, every_layer=False):
    """the method of test_every_group_per_element for any (model, options) -> {group: worst |err| / bound}"""
    no, nop = head_width(m), head_width_padded(m)
    ops.model_load(m.to_blob(), precision=prec, **kw)
    plan = ops.debug_plan(h, w)
    if plan_check is not None:
        plan_check(plan)
    x = _tiles(1000 + h + w + B, B, h, w, m.ch)
    xd = torch.as_tensor(x).cuda()
    info = ops.model_info(h, w)
    assert info["nc"] == m.nc and info["ch"] == m.ch
    g = bounds.Guarded((B, info["anchors"], nop), torch.float32)
    ops.forward(xd, out=g.out)
    torch.cuda.synchronize()
    assert g.guards_intact(), label + "write outside the head tensor"
    head = g.out.clone()
    assert bool(torch.isfinite(head[..., :no]).all()), label + "head element not written or not finite"

    obs = _observe(ops, m, plan, head, x, B, h, w)
    ev = fr.Evaluator(m, prec, obs)
    outputs = [k for k in obs if k != "tile"]
    ratios, covered, single, keep, tw = {}, set(), {}, None, ev.twin()
    for name in outputs:  # forward_ref.check_all, keeping which groups are single-layer and the worst group's reference for the replay
        ref, E, rec = fr.group_bound(ev, name, tw)  # (refuses a group whose bound is vacuous: it cannot count towards the coverage below)
        members = sorted(rec)
        what = f"{label}{name} <- [{len(members)}] {'+'.join(n.replace('model.', '') for n in members if n != name)}"
        ratios[name] = fr.check_group(what, obs[name], ref, E)
        covered |= rec
        if sum(r in m.convs for r in rec) <= 1:
            single[name] = ratios[name]
        if keep is None or ratios[name] >= ratios[keep[0]]:
            keep = (name, ref, E)
    assert len(m.convs) == 96 and {c for c in covered if c in m.convs} == set(m.convs), set(m.convs) - covered
    assert {"attn:model.10.m.0.attn", "up:up13", "up:up16", "pool:model.9.pool0", "pool:model.9.pool1", "pool:model.9.pool2"} <= covered, covered
    assert all(n in ratios for i in range(3) for n in fr.head_names(i))
    for i in range(3):  # every column [0, 65 + nc) of every anchor of the level
        assert sum(obs[n].shape[1] for n in fr.head_names(i)) == no and obs[fr.head_names(i)[0]].shape[2:] == (h // (8 << i), w // (8 << i))
    if every_layer:  # nothing but the tabled in-place tensors is missing
        assert set(m.convs) - set(obs) == _stale(plan), set(m.convs) - set(obs)
    worst, ref, E = keep
    ws = max(single, key=single.get)
    print(f"{label}{len(outputs)} groups, worst ratio {ratios[worst]:.3f} at {worst}; single-layer {single[ws]:.3f} at {ws}", flush=True)

    # replay on a side stream (where the engine captures and launches a hipGraph, or falls back to eager launches): identical either way
    g.raw.fill_(0xFF)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.forward(xd, out=g.out)
    st.synchronize()
    torch.cuda.synchronize()
    assert g.guards_intact(), label + "replay: write outside the head tensor"
    assert torch.equal(g.out[..., :no].view(torch.int32), head[..., :no].view(torch.int32)), label + "replay: head not bit-identical"
    if fr.is_head(worst):
        again = _head_obs(m, g.out.cpu(), h, w)[worst]
    elif worst == "model.10.a":
        again = _read(ops, m, "model.10.cv1", B, h, w)[:, :m.psa_c]
    else:
        again = _read(ops, m, worst, B, h, w)
    fr.check_group(label + "replay " + worst, again, ref, E)
    return ratios


# ---------------------------------------------------------------------------------------------- s, fp32
S_SHAPES = [(64, 96, 3), (128, 160, 2), (416, 416, 1)]


def _assert_one_kernel_per_layer(plan, pw32):
    assert all(l.startswith(("conv32 ", "pw32 ", "dwconv ", "pool ", "upsample ", "attn ", "total_macs")) for l in plan), plan
    assert _count(plan, start="conv32 ") + _count(plan, start="pw32 ") == 96 - 7  # every dense conv of the blob (7 records are depthwise)
    assert _count(plan, start="pw32 ") == pw32 and _count(plan, start="dwconv ") == 7 and _count(plan, start="pool ") == 3, plan
    assert _count(plan, start="upsample ") == 2 and _count(plan, start="attn ") == 1, plan
    assert not _fused_tails(plan) and not any(" vcat1" in l or " upacc1" in l or "|" in l or "+model." in l for l in plan), plan


@pytest.mark.parametrize("h,w,B", S_SHAPES, ids=str)
def test_s_fp32_every_layer_on_its_own(ops, h, w, B):
    """single-layer groups only: the tightest bound the method has, for every layer of the s widths"""
    m = _model("s", 12, 3)
    _per_element(ops, m, "f32", PER_LAYER, h, w, B, f"f32 per-layer s {h}x{w} B{B}: ", every_layer=True,
                 plan_check=lambda plan: _assert_one_kernel_per_layer(plan, pw32=34))


# the default fp32 plan of s nc 12, as debug_plan prints it: (pw32 lines, ` NC2 ` lines, dwconv lines) per tile shape
S_DEFAULT = {(64, 96): (31, 6, 7), (128, 160): (30, 6, 6), (416, 416): (28, 17, 4), (64, 64): (31, 6, 7)}


def _assert_s_default_forms(plan, h, w):
    pw, nc2, dw = S_DEFAULT[h, w]
    assert (_count(plan, start="pw32 "), _count(plan, " NC2 "), _count(plan, start="dwconv ")) == (pw, nc2, dw), plan
    assert _count(plan, " cout32 ", start="stem32 model.0 ") == 1 and _count(plan, start="c3k2f32 ") == 0, plan
    assert _count(plan, " vcat1 ") == 2 and _count(plan, " upacc1 ") == 2 and _count(plan, ".up ", " raw1 ", start="pw32 ") == 2, plan
    assert _count(plan, start="pool sppf.pools ") == 1 and _count(plan, start="pool ") == 1, plan
    assert len(_fused_tails(plan)) == 7 and _count(plan, "|") == 3 and _count(plan, " nh4 ", start="attn ") == 1, plan
    # cin 1024 > 512: model.9.cv2 is beyond k_pw_f32 and runs on k_conv_f32; the 512-input 1x1s take the 16-wave form of k_pw_f32
    assert _count(plan, " cin1024 ", start="conv32 model.9.cv2 ") == 1 and not any(l.startswith("pw32 model.9.cv2 ") for l in plan), plan
    assert _count(plan, " cin512 ", " waves16 ", start="pw32 model.9.cv1 ") == 1 and _count(plan, " cin512 ", " waves16 ", start="pw32 model.10.cv2 ") == 1, plan
    assert _count(plan, " cout12 ", " TW512 ", start="conv32 model.23.cv3.") == 3, plan  # the 128-wide class branch: its logit conv is a launch of its own


@pytest.mark.parametrize("ch,h,w,B", [(3,) + s for s in S_SHAPES] + [(4, 64, 64, 2)], ids=str)
def test_s_fp32_default_plan(ops, ch, h, w, B):
    m = _model("s", 12, ch)
    _per_element(ops, m, "f32", {}, h, w, B, f"f32 default s ch{ch} {h}x{w} B{B}: ", plan_check=lambda plan: _assert_s_default_forms(plan, h, w))


S_NAMED = ("x2", "x4", "x16", "x19", "model.2.cv2", "model.4.cv2", "model.6.cv2", "model.8.cv2", "model.9.cv2", "model.10.m.0.attn.qkv", "model.10.m.0.ffn.1",
           "model.10.cv2", "model.13.cv1", "model.13.cv2", "model.16.cv1", "model.16.cv2", "model.19.cv2", "model.22.cv1", "model.22.cv2")


def _head_and_taps(ops, m, kw, x, B, h, w, names=S_NAMED):
    ops.model_load(m.to_blob(), precision="f32", **kw)
    plan = ops.debug_plan(h, w)
    head = ops.forward(x)[..., :head_width(m)].cpu()
    return plan, head, {n: ops.debug_activation(n, B, h, w).cpu() for n in names}


def _assert_same(tag, a, b):
    assert torch.equal(a[1], b[1]), f"{tag}: heads differ, max {float((a[1] - b[1]).abs().max())}"
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), f"{tag}: {n} differs, max {float((a[2][n] - b[2][n]).abs().max())}"


@pytest.mark.parametrize("h,w,B", [(64, 96, 3), (416, 416, 1)], ids=str)
def test_s_fp32_forms_are_bit_identical(ops, h, w, B):
    """device against device, heads and named activations BIT FOR BIT: the fused default plan (stem off on both sides) against one kernel
    per layer, then each of nc2 / blk32 / pw32 / upacc / c3k2f switched off singly against the default"""
    m = _model("s", 12, 3)
    x = torch.as_tensor(_tiles(77 + h + B, B, h, w, 3)).cuda()
    plain = _head_and_taps(ops, m, PER_LAYER, x, B, h, w)
    _assert_one_kernel_per_layer(plain[0], pw32=34)
    fused = _head_and_taps(ops, m, dict(stem=False), x, B, h, w)
    assert len(_fused_tails(fused[0])) == 7 and _count(fused[0], " vcat1 ") == 2 and _count(fused[0], " upacc1 ") == 2 and _count(fused[0], "|") == 3, fused[0]
    assert _count(fused[0], start="pool sppf.pools ") == 1 and not any(l.startswith("stem32 ") for l in fused[0]), fused[0]
    _assert_same("default (stem off) vs one kernel per layer", plain, fused)

    base = _head_and_taps(ops, m, {}, x, B, h, w)
    _assert_s_default_forms(base[0], h, w)
    npw, nnc2, _ = S_DEFAULT[h, w]
    for key in ("nc2", "blk32", "pw32", "upacc", "c3k2f"):
        off = _head_and_taps(ops, m, {key: False}, x, B, h, w)
        if key == "nc2":  # (the two-launch upacc form needs the two-fragment conv: it goes with it, and with it the two `.up` launches)
            assert _count(off[0], " NC2 ") == 0 and _count(off[0], " upacc1 ") == 0 and _count(off[0], start="pw32 ") == npw - 2, off[0]
        if key == "pw32":  # every 1x1 on k_conv_f32 (and no `.up` launch, which is a k_pw_f32 form)
            assert _count(off[0], start="pw32 ") == 0 and _count(off[0], start="conv32 ") == 78 and _count(off[0], " upacc1 ") == 0, off[0]
        if key == "upacc":
            assert _count(off[0], " upacc1 ") == 0 and _count(off[0], " vcat1 ") == 2 and _count(off[0], start="pw32 ") == npw - 2, off[0]
        if key == "blk32":  # a change of addresses only: the same launches
            assert [l.split()[:2] for l in off[0]] == [l.split()[:2] for l in base[0]]
        if key == "c3k2f":  # nothing to switch at s (module docstring): the plans are equal
            assert off[0] == base[0]
        _assert_same(f"{key} off vs default", base, off)


def test_s_fp32_resident_workgroups_are_bit_identical(ops):
    """`xtile` at s: 300 tiles of 64 x 64 are more tiles than resident workgroups in most layers"""
    m = _model("s", 12, 3)
    h = w = 64
    B = 300
    x = torch.as_tensor(_tiles(7, B, h, w, 3)).cuda()
    ops.model_load(m.to_blob(), precision="f32", xtile=False)
    one = ops.forward(x)[..., :77].cpu()
    ops.model_load(m.to_blob(), precision="f32")
    res = ops.forward(x)[..., :77].cpu()
    assert torch.equal(one, res), float((one - res).abs().max())
    small = ops.forward(x[137:139].contiguous())[..., :77].cpu()  # and the same tiles in a small batch of their own (never resident)
    assert torch.equal(res[137:139], small)


def test_s_fp32_nc15(ops):
    """a 128-wide class branch, a partial class slice and an unaligned angle column (79) together; 65 + nc == padded width"""
    m = _model("s", 15, 3)
    assert head_width(m) == head_width_padded(m) == 80

    def check(plan):
        assert _count(plan, " cin128 ", " cout15 ", " tail0 ", start="conv32 model.23.cv3.") == 3, plan
        assert len([l for l in _fused_tails(plan) if " tail1 " in l and ".cv4." in l]) == 3, plan
    _per_element(ops, m, "f32", {}, 64, 96, 2, "f32 default s nc15 64x96 B2: ", plan_check=check)


# ---------------------------------------------------------------------------------------------- class counts, n, fp32
def _assert_n_fp32_head(plan, nc, tail=True):
    cls = [l for l in plan if l.startswith("conv32 ") and any(f"model.23.cv3.{i}.2 " in l for i in range(3))]
    assert len(cls) == 3 and _count(plan, start="c3k2f32 ") == (1 if tail else 0), plan
    if not tail:  # the logit conv as a launch of its own into the same slices
        assert all(f" cin64 cout{nc} " in l and " tail0 " in l and "+model." not in l for l in cls) and not _fused_tails(plan), plan
    elif nc <= 64:  # c3 = 64: the logit conv rides behind cv3.i.1.1 (` tailN `, N = nc)
        assert all(f".1.1+model.23.cv3.{i}.2 " in l and f" tail{nc} " in l for i, l in enumerate(cls)) and len(_fused_tails(plan)) == 11, plan
    else:  # c3 = 80: no pw32 (cout % 64), no fused tail (cout2 <= 64)
        assert all(" cin80 cout80 " in l and " tail0 " in l and "+model." not in l for l in cls) and len(_fused_tails(plan)) == 8, plan
        assert _count(plan, start="pw32 ") == 27 and not any(l.startswith("pw32 model.23.cv3.") for l in plan), plan


NC_CASES = [(nc, 3, True, 64, 96, 3) for nc in (1, 13, 15, 16, 80)] + [(nc, 3, True, h, w, B) for nc in (13, 80) for (h, w, B) in ((416, 416, 1), (128, 128, 5))] + \
           [(13, 4, True, 64, 96, 3), (13, 3, False, 64, 96, 3)]


@pytest.mark.parametrize("nc,ch,tail,h,w,B", NC_CASES, ids=str)
def test_class_counts_fp32(ops, nc, ch, tail, h, w, B):
    m = _model("n", nc, ch)
    assert m.head_c[1] == (80 if nc == 80 else 64)
    _per_element(ops, m, "f32", {} if tail else dict(tail=False), h, w, B, f"f32 {'default' if tail else 'tail=False'} n nc{nc} ch{ch} {h}x{w} B{B}: ",
                 plan_check=lambda plan: _assert_n_fp32_head(plan, nc, tail))


# ---------------------------------------------------------------------------------------------- class counts, 16 bit
def _assert_dwpw(plan, nc, h, w):
    """dwpw (depthwise 3x3 + 1x1 in one launch) carries the head's logit conv as a fused tail only for tail_cout % 4 == 0, <= 16"""
    dwpw = [l for l in plan if l.startswith("dwpw ")]
    if (h, w) == (64, 96):  # maps of 8x12 / 4x6 / 2x3: no level takes the form
        assert not dwpw, plan
    elif nc == 16:
        assert len(dwpw) == 4 and sorted(f".1.1+model.23.cv3.{i}.2 " in l and " tail16 " in l for i in (0, 1) for l in dwpw) == [False] * 6 + [True] * 2, plan
    elif nc in (13, 20):  # falls back: the pair without the tail
        assert len(dwpw) == 2 and all(" tail0 " in l and ".0.0+model.23.cv3." in l for l in dwpw), plan
    else:  # nc 80: c3 = 80 is outside the form altogether
        assert nc == 80 and not dwpw, plan
    assert not any(" tail" in l and " tail0 " not in l and " tail16 " not in l for l in dwpw), plan


@pytest.mark.parametrize("h,w,B", [(416, 416, 1), (64, 96, 3)], ids=str)
@pytest.mark.parametrize("nc", [13, 16, 20, 80])
@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_class_counts_16bit(ops, prec, nc, h, w, B):
    m = _model("n", nc, 3)
    _per_element(ops, m, prec, {}, h, w, B, f"{prec} default n nc{nc} {h}x{w} B{B}: ", plan_check=lambda plan: _assert_dwpw(plan, nc, h, w))


# ---------------------------------------------------------------------------------------------- the gate
@pytest.mark.parametrize("nc", [13, 15])
def test_gate_is_the_exact_class_maximum(ops, nc):
    """ops.forward(..., cmax=): cmax == max over the class logits of the SAME head, exactly, for every anchor (an angle or a padding
    column inside the maximum, or a class column outside it, cannot hide); the head equals the ungated call bit for bit"""
    m = _model("n", nc, 3)
    h, w, B = 64, 96, 3
    no, nop = head_width(m), head_width_padded(m)
    ops.model_load(m.to_blob(), precision="f32")
    xd = torch.as_tensor(_tiles(5 + nc, B, h, w, 3)).cuda()
    A = ops.model_info(h, w)["anchors"]
    plain = ops.forward(xd).clone()
    g, c = bounds.Guarded((B, A, nop), torch.float32), bounds.Guarded((B, A), torch.float32)
    ops.forward(xd, out=g.out, cmax=c.out)
    torch.cuda.synchronize()
    assert g.guards_intact() and c.guards_intact(), "write outside the head or the gate tensor"
    assert bool(torch.isfinite(c.out).all()), "gate element not written"
    assert torch.equal(g.out[..., :no].view(torch.int32), plain[..., :no].view(torch.int32)), "gated head differs from the ungated one"
    assert torch.equal(c.out, g.out[..., 64:64 + nc].max(-1).values), float((c.out - g.out[..., 64:64 + nc].max(-1).values).abs().max())
