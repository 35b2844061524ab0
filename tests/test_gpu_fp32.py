"""fp32-arithmetic mode (obb_set_option "precision" = 32) against the fp32 torch-CPU oracle -- what the reference computes
(Detect_OBB.py:79-83: model(net_input, conf=...) with Ultralytics' default half=False).

Unlike tests/test_gpu_pipeline.py nothing is injected here: the oracle pipeline runs ITS OWN fp32 forward (one tile per call,
like the reference) and the device runs its own; the detection lists must agree one to one.  The same comparison for the 16-bit
default states the detection-set agreement of the fp16 path as tested numbers."""
import numpy as np
import pytest
import torch

from oracle import geom as og
from oracle import pipeline as opl
from oracle.yolo11_obb import Yolo11OBB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ood():
    assert torch.cuda.is_available()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import detect, model, ops

    class NS:
        pass
    ns = NS()
    ns.detect, ns.model, ns.ops = detect, model, ops
    return ns


@pytest.fixture(scope="module")
def nets():
    return {416: Yolo11OBB("n", nc=12, ch=3, seed=0), 128: Yolo11OBB("n", nc=12, ch=3, seed=1)}


def _tiles(seed, B, h, w, ch=3):
    return np.random.default_rng(seed).integers(0, 256, (B, h, w, ch), dtype=np.uint8)


TAPS = ["model.0", "model.1", "model.2.cv1", "model.2.m.0.cv1", "model.2.m.0.cv2", "model.2.cv2", "model.3", "model.4.cv2", "model.5",
        "model.6.m.0.cv3", "model.6.cv2", "model.7", "model.8.cv2", "model.9.cv1", "model.9.cv2", "model.10.cv1", "model.10.m.0.attn.qkv",
        "model.10.m.0.attn", "model.10.m.0.attn.pe", "model.10.m.0.ffn.1", "model.10.cv2", "model.13.cv2", "model.16.cv2", "model.17",
        "model.19.cv2", "model.20", "model.22.cv2", "model.23.cv2.0.1", "model.23.cv3.0.0.0", "model.23.cv3.0.1.1", "model.23.cv4.2.1"]


def test_fp32_layer_taps(ood, nets):
    """every layer of the fp32 plan (one kernel per layer) vs the fp32 oracle: both sides are fp32 fma chains, only the order differs"""
    ops, net = ood.ops, nets[416]
    x = _tiles(1, 2, 416, 416)
    taps = {}
    net.forward_raw(x, "fp32", taps)
    ops.model_load(net.to_blob(), precision="f32", tail=False, upfold=False, sppf_fuse=False, stem=False)  # one generic kernel per layer: every activation exists
    plan = ops.debug_plan(416, 416)
    assert all(l.startswith(("conv32 ", "pw32 ", "dwconv ", "pool ", "upsample ", "attn ", "total_macs")) for l in plan), plan
    assert sum(l.startswith(("conv32 ", "pw32 ")) for l in plan) == 96 - 7  # every dense conv of the blob (7 records are depthwise)
    assert sum(l.startswith("pw32 ") for l in plan) >= 20                   # (the 1x1 layers with >= 64 input channels: k_pw_f32)
    assert not any(" tail" in l and " tail0 " not in l for l in plan if l.startswith("conv32 ")) and not any(" vcat1" in l for l in plan)
    ops.forward(torch.as_tensor(x).cuda())
    torch.cuda.synchronize()
    for name in TAPS:
        got = ops.debug_activation(name, 2, 416, 416).cpu()
        exp = taps[name].permute(0, 2, 3, 1)
        if name == "model.10.m.0.attn.qkv":  # device stores [q heads | k heads | v heads]
            nh, kd, hd = 2, 32, 64
            idx = [h * (2 * kd + hd) + d for h in range(nh) for d in range(kd)] + [h * (2 * kd + hd) + kd + d for h in range(nh) for d in range(kd)] + \
                  [h * (2 * kd + hd) + 2 * kd + d for h in range(nh) for d in range(hd)]
            exp = exp[..., idx]
        assert got.shape == exp.shape, name
        if name == "model.10.cv1":  # the b half is updated in place by the PSA block
            got, exp = got[..., :128], exp[..., :128]
        d = (got - exp).abs()
        scale = float(exp.abs().mean())
        print(name, "max", float(d.max()), "mean", float(d.mean()), "scale", scale, flush=True)
        assert float(d.max()) < 1e-3 and float(d.mean()) < 2e-5, name  # measured: mean 1e-7 (model.0) .. 5e-6 (head), max <= 1e-4


@pytest.mark.parametrize("h,w,B", [(416, 416, 3), (128, 128, 5), (416, 288, 2), (64, 96, 3)])
def test_fp32_fused_forms_are_bit_identical(ood, nets, h, w, B):
    """The default fp32 plan (trailing 1x1 convs fused behind their producers, Upsample + Concat read in place, merged sibling convs, the
    three SPPF pools in one launch) against the one-kernel-per-layer plan: every fused form keeps the k order of the layer it replaces
    (the exact-f32 MFMA is a k-ordered fma chain) and max pooling is exact, so the heads must agree BIT FOR BIT."""
    ops, net = ood.ops, nets[416]
    x = torch.as_tensor(_tiles(3 + h, B, h, w)).cuda()
    ops.model_load(net.to_blob(), precision="f32", tail=False, upfold=False, sppf_fuse=False, stem=False)
    plain = ops.forward(x).cpu()
    x0_plain = ops.debug_activation("model.0", B, h, w).cpu()
    ops.model_load(net.to_blob(), precision="f32", stem=False)
    plan = ops.debug_plan(h, w)
    assert any(" tail64 " in l for l in plan) and any(" vcat1 " in l for l in plan) and any("|" in l for l in plan) and any("sppf" in l for l in plan), plan
    assert sum(l.startswith("c3k2f32 ") for l in plan) == 1, plan  # Bottleneck + closing 1x1 of model.2 in one launch (c3k2f32.hip)
    fused = ops.forward(x).cpu()
    x2_plain_vs = ops.debug_activation("model.2.cv2", B, h, w).cpu()
    assert torch.equal(fused[..., :77], plain[..., :77]), float((fused - plain)[..., :77].abs().max())
    ops.model_load(net.to_blob(), precision="f32", stem=False, c3k2f=False)  # the block kernel alone off: its output tensor, bit for bit
    assert not any(l.startswith("c3k2f32 ") for l in ops.debug_plan(h, w))
    ops.forward(x)
    assert torch.equal(ops.debug_activation("model.2.cv2", B, h, w).cpu(), x2_plain_vs)
    # two forms that sum in another order than what they replace: close, not identical
    # (a) the MFMA attention core vs the scalar one
    ops.model_load(net.to_blob(), precision="f32", attn_mfma=False, stem=False)
    scalar = ops.forward(x).cpu()
    d = (scalar - fused)[..., :77].abs()
    print(h, w, "attention mfma vs scalar: max", float(d.max()), "mean", float(d.mean()))
    assert float(d.max()) < 5e-4 and float(d.mean()) < 1e-5
    # (b) the row-stripe input layer (k dense over the 27 taps) vs the generic kernel (4-channel chunks per tap)
    ops.model_load(net.to_blob(), precision="f32")
    assert any(l.startswith("stem32 ") for l in ops.debug_plan(h, w))
    full = ops.forward(x).cpu()
    x0 = ops.debug_activation("model.0", B, h, w).cpu()
    d0, d = (x0 - x0_plain).abs(), (full - fused)[..., :77].abs()
    print(h, w, "stem stripes vs generic: model.0 max", float(d0.max()), "head max", float(d.max()), "mean", float(d.mean()))
    assert float(d0.max()) < 2e-6 * max(1.0, float(x0_plain.abs().max())) and float(d.max()) < 5e-4 and float(d.mean()) < 3e-5


@pytest.mark.parametrize("h,w,B", [(416, 416, 5), (128, 128, 33), (416, 288, 2), (64, 96, 3), (416, 416, 40)])
def test_fp32_two_fragment_form_is_bit_identical(ood, nets, h, w, B):
    """`nc2`: a wave of the conv kernel owning two cout fragments x <= 4 pixel fragments (a third fewer LDS operand reads, 32-byte stores per
    lane) against one x <= 7 -- every output still sums its k in the same order, so the heads must agree BIT FOR BIT (the weight rows are
    permuted on the host to the interleaved cout order of the form: a wrong permutation cannot hide)."""
    ops, net = ood.ops, nets[416]
    x = torch.as_tensor(_tiles(11 + h + B, B, h, w)).cuda()
    ops.model_load(net.to_blob(), precision="f32", nc2=False)
    assert not any(" NC2 " in l for l in ops.debug_plan(h, w))
    one = ops.forward(x).cpu()
    for kw, least in ((dict(pw32=False), 10), ({}, 1)):  # (the 1x1 layers with >= 64 input channels go to k_pw_f32 by default)
        ops.model_load(net.to_blob(), precision="f32", **kw)
        assert sum(" NC2 " in l for l in ops.debug_plan(h, w)) >= least, ops.debug_plan(h, w)
        two = ops.forward(x).cpu()
        assert torch.equal(one[..., :77], two[..., :77]), float((one - two)[..., :77].abs().max())


@pytest.mark.parametrize("h,w,B,ch", [(416, 416, 5, 3), (128, 128, 33, 3), (416, 288, 2, 3), (64, 96, 3, 3), (416, 416, 3, 4)])
def test_fp32_channel_blocked_buffers_are_bit_identical(ood, nets, h, w, B, ch):
    """`blk32`: the tensors read by 3x3 convs in 8- / 16-channel stages (x2, x4, x6, x16, x19, the first convs of the box branch) stored as
    8-channel blocks per image instead of plain NHWC -- a pure change of addresses (the stage then reads dense runs instead of 32-byte pieces
    of wide pixel rows): heads BIT FOR BIT, and the named activations read back through the blocked layout equal the plain ones."""
    ops = ood.ops
    net = nets[416] if ch == 3 else Yolo11OBB("n", nc=12, ch=4, seed=3)
    x = torch.as_tensor(_tiles(23 + h + B, B, h, w, ch)).cuda()
    ops.model_load(net.to_blob(), precision="f32", blk32=False)
    plain = ops.forward(x).cpu()
    taps = {n: ops.debug_activation(n, B, h, w).cpu() for n in ("x2", "x4", "x16", "x19")}
    ops.model_load(net.to_blob(), precision="f32")
    blocked = ops.forward(x).cpu()
    assert torch.equal(plain[..., :77], blocked[..., :77]), float((plain - blocked)[..., :77].abs().max())
    for n, t in taps.items():
        assert torch.equal(t, ops.debug_activation(n, B, h, w).cpu()), n


@pytest.mark.parametrize("h,w,B,ch", [(416, 416, 5, 3), (128, 128, 70, 3), (416, 288, 2, 3), (64, 96, 3, 3), (416, 416, 2, 4)])
def test_fp32_direct_operand_1x1_is_bit_identical(ood, nets, h, w, B, ch):
    """`pw32`: the 1x1 layers with >= 64 input channels on k_pw_f32 (weights of a 64-cout block resident in LDS, a lane's B operand loaded straight
    from global memory, no activation staging, no barrier in the k loop) against k_conv_f32 (both operands staged through LDS): the same k order
    (16-channel pieces, element s inside), the same epilogue -- heads and named 1x1 outputs BIT FOR BIT, incl. the residual layers of C2PSA, the
    permuted qkv rows and the 8-channel-blocked outputs."""
    ops = ood.ops
    net = nets[416] if ch == 3 else Yolo11OBB("n", nc=12, ch=4, seed=3)
    x = torch.as_tensor(_tiles(31 + h + B, B, h, w, ch)).cuda()
    names = ("model.4.cv2", "model.6.cv2", "model.8.cv2", "model.9.cv2", "model.10.m.0.attn.qkv", "model.10.m.0.ffn.1", "model.10.cv2", "model.13.cv2", "model.19.cv2", "model.22.cv2")
    ops.model_load(net.to_blob(), precision="f32", pw32=False)
    assert not any(l.startswith("pw32 ") for l in ops.debug_plan(h, w))
    staged = ops.forward(x).cpu()
    taps = {n: ops.debug_activation(n, B, h, w).cpu() for n in names}
    ops.model_load(net.to_blob(), precision="f32")
    assert sum(l.startswith("pw32 ") for l in ops.debug_plan(h, w)) >= 20, ops.debug_plan(h, w)
    direct = ops.forward(x).cpu()
    for n, t in taps.items():
        assert torch.equal(t, ops.debug_activation(n, B, h, w).cpu()), n
    assert torch.equal(staged[..., :77], direct[..., :77]), float((staged - direct)[..., :77].abs().max())


def test_rounds_are_sized_by_pixels_and_do_not_change_results(ood, nets):
    """A round of the forward holds 1024 tiles of 416 x 416 or proportionally more smaller ones (at most 16 384): 16 400 tiles of 64 x 64 are two
    equal rounds of 8200; every tile's head must equal what the same tile gives in a small batch of its own."""
    ops, net = ood.ops, nets[416]
    ops.model_load(net.to_blob(), precision="f32")
    B = 16400
    x = torch.as_tensor(_tiles(99, B, 64, 64)).cuda()
    full = ops.forward(x).clone()
    for lo, hi in ((0, 5), (8195, 8205), (16387, 16400), (4000, 4003)):
        part = ops.forward(x[lo:hi].contiguous())
        assert torch.equal(full[lo:hi, :, :77], part[..., :77]), (lo, hi)


@pytest.mark.parametrize("h,w,B", [(416, 416, 40), (128, 128, 600), (192, 416, 37)])
def test_fp32_resident_workgroups_are_bit_identical(ood, nets, h, w, B):
    """`xtile`: conv workgroups that stay resident and walk several tiles (next tile's first stage fetched under this tile's last k loop)
    against one tile per workgroup -- the same arithmetic in the same order, so the heads must agree BIT FOR BIT.  The batch is large
    enough for more tiles than resident workgroups in most layers (a small batch never takes the resident form)."""
    ops, net = ood.ops, nets[416]
    x = torch.as_tensor(_tiles(7 + h, B, h, w)).cuda()
    ops.model_load(net.to_blob(), precision="f32", xtile=False)
    one = ops.forward(x).cpu()
    ops.model_load(net.to_blob(), precision="f32")
    res = ops.forward(x).cpu()
    assert torch.equal(one[..., :77], res[..., :77]), float((one - res)[..., :77].abs().max())


@pytest.mark.parametrize("h,w,B,ch", [(416, 416, 3, 3), (128, 128, 5, 3), (416, 288, 2, 3), (192, 416, 2, 3), (64, 96, 3, 3), (416, 416, 2, 4)])
def test_fp32_head_matches_fp32_oracle(ood, nets, h, w, B, ch):
    ops = ood.ops
    net = nets[416] if ch == 3 else Yolo11OBB("n", nc=12, ch=4, seed=3)
    ops.model_load(net.to_blob(), precision="f32")
    x = _tiles(10 + h + w, B, h, w, ch)
    head = ops.forward(torch.as_tensor(x).cuda()).cpu()[..., :77]
    ref = net.forward_raw(x, "fp32")
    ref64 = net.forward_raw(x, "fp64")
    d = (head - ref).abs()
    conf_d = (torch.sigmoid(head[..., 64:76]) - torch.sigmoid(ref[..., 64:76])).abs()
    e_dev, e_ref = (head.double() - ref64).abs(), (ref.double() - ref64).abs()
    print(h, w, ch, "vs torch fp32: logit max/mean", float(d.max()), float(d.mean()), "conf max", float(conf_d.max()),
          "| vs fp64: device max/mean", float(e_dev.max()), float(e_dev.mean()), "torch-fp32 max/mean", float(e_ref.max()), float(e_ref.mean()))
    # two fp32 evaluations of a 23-layer network differ by their summation orders; the yardstick is the double-precision evaluation of the
    # same fp32 weights: the device must sit as close to it as torch's own fp32 forward does (and both stay inside absolute caps)
    assert float(e_dev.mean()) <= 1.5 * float(e_ref.mean()) + 1e-7 and float(e_dev.max()) <= 2.0 * float(e_ref.max()) + 1e-6
    assert float(d.max()) < 2e-3 and float(d.mean()) < 5e-5 and float(conf_d.max()) < 2e-4
    # deterministic and batch-invariant like the 16-bit path
    again = ops.forward(torch.as_tensor(x).cuda()).cpu()[..., :77]
    one = ops.forward(torch.as_tensor(x[1:2]).cuda()).cpu()[..., :77]
    assert torch.equal(again, head) and torch.equal(one[0], head[1])


def _same_dets(got, exp, conf_tol, px_tol, tag="", max_subst=0, max_flips=0):
    """identical count; one-to-one correspondence (same class, every corner within px_tol, confidence within conf_tol); identical ORDER
    except between detections whose confidences are closer than 2 * conf_tol (the lists are confidence-sorted: two fp32 evaluations may
    legitimately swap near-ties).  max_subst > 0 additionally tolerates that many SUBSTITUTIONS between NMS rivals in a near-tie: the two
    evaluations kept different members of a pair of overlapping same-class candidates (polygon IoU >= 0.3) whose confidences differ by
    less than 2 * conf_tol -- which of the two survives the NMS is decided by the last bits of their scores.  max_flips > 0 tolerates that
    many detections present on one side only (a hard threshold -- confidence 0.25 / 0.70, merge IoU 0.4 -- crossed by the last bits of one
    evaluation): they are removed from the comparison after being reported; everything else must still correspond one to one."""
    if len(got) != len(exp) or max_flips:
        # pair off what corresponds, set the few one-sided detections aside
        used_e, keep_g = set(), []
        for gi, g in enumerate(got):
            j = next((j for j, e in enumerate(exp) if j not in used_e and e[8] == g[8] and max(abs(a - b) for a, b in zip(g[:8], e[:8])) <= max(px_tol, 0.5)), None)
            if j is None:
                print(f"{tag}: only on the device: class {g[8]} conf {g[9]:.6f}")
            else:
                used_e.add(j)
                keep_g.append(gi)
        only_e = [j for j in range(len(exp)) if j not in used_e]
        for j in only_e:
            print(f"{tag}: only in the reference: class {exp[j][8]} conf {exp[j][9]:.6f}")
        flips = (len(got) - len(keep_g)) + len(only_e)
        assert flips <= max_flips, (len(got), len(exp), flips)
        if flips:
            got = [got[i] for i in keep_g]
            exp = [e for j, e in enumerate(exp) if j in used_e]
    assert len(got) == len(exp), (len(got), len(exp))
    used, pos = set(), []
    dc = dp = da = 0.0
    subst = []
    for gi, g in enumerate(got):
        best, bj = None, -1
        for j, e in enumerate(exp):
            if j in used or e[8] != g[8]:
                continue
            d = max(abs(a - b) for a, b in zip(g[:8], e[:8]))
            if best is None or d < best:
                best, bj = d, j
        assert bj >= 0, g
        if best > px_tol:
            subst.append(gi)
            pos.append(None)
            continue
        used.add(bj)
        pos.append(bj)
        dc, dp, da = max(dc, abs(g[9] - exp[bj][9])), max(dp, best), max(da, abs(g[10] - exp[bj][10]))
    assert len(subst) <= max_subst, ("unmatched detections", [(got[i], ) for i in subst][:3])
    for gi in subst:  # each must be the NMS rival of a still unmatched reference detection
        g = got[gi]
        cand = [(og.compute_polygon_iou(list(g[:8]), list(e[:8])), j) for j, e in enumerate(exp) if j not in used and e[8] == g[8] and abs(e[9] - g[9]) <= 2 * conf_tol]
        assert cand and max(cand)[0] >= 0.3, ("not a near-tie between NMS rivals", g, cand)
        j = max(cand)[1]
        used.add(j)
        pos[gi] = j
        print(f"{tag}: near-tie substitution: device kept conf {g[9]:.6f}, reference kept conf {exp[j][9]:.6f}, IoU of the two {max(cand)[0]:.3f}")
    swaps = 0
    for i, j in enumerate(pos):
        if i != j:
            swaps += 1
            assert abs(exp[i][9] - exp[j][9]) <= 2 * conf_tol, ("order differs beyond a near-tie", i, j, exp[i][9], exp[j][9])
    print(f"{tag}: {len(got)} detections, identical count / classes; {swaps} positions permuted among near-ties; {len(subst)} near-tie substitutions; "
          f"max |d conf| {dc:.2e}, max |d corner| {dp:.2e} px, max |d angle| {da:.2e} deg")
    assert dc <= conf_tol and da <= 0.1


def test_fp32_detect_symbols_end_to_end(ood, nets):
    """807 x 895 image (the Test1 grid: 4 full + 5 partial tiles incl. the resized corner), NO head injection: identical count, class
    and order; confidences <= 2e-4; corners <= 0.1 px (both are the propagated summation-order noise of fp32, see the fp64 yardstick above:
    a head logit moves by up to ~5e-4, a DFL distance by that times the stride)."""
    img = np.random.default_rng(7).integers(0, 256, (807, 895, 3), dtype=np.uint8)
    model = ood.model.YOLO(nets[416], imgsz=416, precision="f32")
    exp = opl.detect_symbols(img, opl.OracleModel(nets[416], 416, "fp32"), 416, 100)
    got = ood.detect.detect_symbols(img, model, 416, 100)
    assert len(exp) > 5
    _same_dets(got, exp, 2e-4, 0.1, "fp32 detect_symbols 807x895")


def _thin_tile_rows(img, om, tile, overlap):
    """rows the oracle's own model call gives on the thin crops (<= 10 px) of the grid: -> (from wide-and-low crops, from tall-and-narrow ones)"""
    H, W = img.shape[:2]
    hz = vt = 0
    for (x, y, x2, y2) in og.tile_grid(H, W, tile, overlap):
        if (y2 - y <= 10) != (x2 - x <= 10):
            n = len(om.predict_rows(np.ascontiguousarray(img[y:y2, x:x2]), 0.25)[1])
            hz, vt = hz + (n if y2 - y <= 10 else 0), vt + (n if x2 - x <= 10 else 0)
    return hz, vt


@pytest.mark.parametrize("key,H,W,tile,overlap,border", [(416, 642, 640, 416, 100, False), (416, 642, 640, 416, 100, True), (128, 206, 204, 128, 30, False)])
def test_fp32_detect_symbols_end_to_end_with_thin_border_tiles(ood, nets, key, H, W, tile, overlap, border):
    """An image whose grid ends in border crops 10 px tall, 8 px wide and the 10 x 8 corner (642 x 640 at 416 / 100, 206 x 204 at 128 / 30):
    LetterBox(auto=True) makes them 32 x 416, 416 x 32 and 416 x 352 (32 x 128, 128 x 32, 128 x 128) network inputs.  Nothing injected;
    comparison and allowances of test_fp32_detect_symbols_end_to_end.  With the reference's border filter (margin 20 / 10 px on every
    side) no detection of a crop below 40 / 20 px can survive, so the thin tiles reach the result only with the filter off: that is the
    configuration in which the oracle's own result is asserted to hold detections of a thin tile of each orientation (the per-tile merge
    keeps at least one of a tile's rows); the default configuration must agree too.
    The 10 x 8 corner has its contrast reduced to 114 +- 24: upscaled 41 times, full-contrast noise puts more than max_det = 300 rows of
    saturated confidence (0.99999 +- 1e-7) into that one tile, and WHICH 300 survive the cap is then decided between bit-identical
    confidences -- measured on MI355X with the full-contrast corner: 822 detections on both sides, all matched but one row displaced at
    the cap (device-only conf 0.9999985, oracle-only conf 0.99977, heads within 2.1e-4, letterbox byte-identical).  The oracle's own row
    count of every thin tile and of the corner is asserted to stay below the cap."""
    img = np.random.default_rng(20).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[H - 10:, W - 8:] = (114 + (img[H - 10:, W - 8:].astype(np.int32) - 128) * 24 // 128).astype(np.uint8)
    shapes = {(int(y2 - y), int(x2 - x)) for (x, y, x2, y2) in og.tile_grid(H, W, tile, overlap)}
    assert {(10, tile), (tile, 8), (10, 8)} <= shapes, shapes
    om = opl.OracleModel(nets[key], tile, "fp32")
    model = ood.model.YOLO(nets[key], imgsz=tile, precision="f32")
    exp = opl.detect_symbols(img, om, tile, overlap, apply_border=border)
    got = ood.detect.detect_symbols(img, model, tile, overlap, ood.detect.Config(APPLY_BORDER_FILTER=border))
    for (x, y, x2, y2) in og.tile_grid(H, W, tile, overlap):
        if y2 - y <= 10 or x2 - x <= 10:
            assert len(om.predict_rows(np.ascontiguousarray(img[y:y2, x:x2]), 0.25)[1]) < om.max_det, (x, y, x2, y2)
    if not border:
        hz, vt = _thin_tile_rows(img, om, tile, overlap)
        print(f"oracle rows from thin tiles: {hz} from 10-px-tall crops, {vt} from 8-px-wide crops; {len(exp)} detections in all")
        assert hz > 0 and vt > 0
    assert len(exp) > 5
    _same_dets(got, exp, 2e-4, 0.1, f"fp32 detect_symbols {H}x{W} tile {tile} border filter {border}")


def test_fp32_four_channel_end_to_end_with_thin_border_tiles(ood):
    """the same 642 x 640 image through a 4-channel checkpoint: the DT-edge channel is built on crops 10 px tall and 8 px wide (above
    build_multich's documented minimum of 2 px) before the letterbox; allowances of test_fp32_four_channel_end_to_end_no_injection"""
    net = Yolo11OBB("n", nc=12, ch=4, seed=2)
    model = ood.model.YOLO(net, imgsz=416, precision="f32")
    img = np.random.default_rng(20).integers(0, 256, (642, 640, 3), dtype=np.uint8)
    om = opl.OracleModel(net, 416, "fp32")
    exp = opl.detect_symbols(img, om, 416, 100, apply_border=False)
    got = ood.detect.detect_symbols(img, model, 416, 100, ood.detect.Config(APPLY_BORDER_FILTER=False))
    hz, vt = _thin_tile_rows(img, om, 416, 100)
    assert hz > 0 and vt > 0 and len(exp) > 5
    _same_dets(got, exp, 2e-4, 0.1, "fp32 4-channel detect_symbols 642x640, border filter off", max_subst=2)


def test_fp32_process_image_dual_scale_end_to_end(ood, nets):
    img = np.random.default_rng(9).integers(0, 256, (500, 640, 3), dtype=np.uint8)
    m128 = ood.model.YOLO(nets[128], imgsz=128, precision="f32")
    m416 = ood.model.YOLO(nets[416], imgsz=416, precision="f32")
    oms = [opl.OracleModel(nets[128], 128, "fp32"), opl.OracleModel(nets[416], 416, "fp32")]
    exp, exp_by_scale = opl.process_image(img, oms)
    got = ood.detect.process_image(img, None, [m128, m416])
    assert sum(len(v) for v in exp_by_scale.values()) > 20 and len(exp) > 3
    _same_dets(got, exp, 2e-4, 0.1, "fp32 dual-scale process_image 500x640")


def test_fp32_four_channel_end_to_end_no_injection(ood):
    """BASELINE configs[3] on one GPU with NO head injection: a 3-channel BGR image, every crop gets its DT-edge channel on the device
    (build_multich) and goes through the device's own fp32 forward; the oracle builds the channel with the numpy restatement (byte-identical to
    the device's, tests/test_gpu_dtedge.py) and runs its own fp32 forward: nothing is shared between the two pipelines but the image.
    Same bounds as the 3-channel comparisons above."""
    net = Yolo11OBB("n", nc=12, ch=4, seed=2)
    model = ood.model.YOLO(net, imgsz=416, precision="f32")
    assert model.ch == 4
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (600, 740, 3), dtype=np.uint8)
    img[100:130, 50:600] = 15
    img[200:520, 300:330] = (240, 10, 10)
    got = ood.detect.detect_symbols(img, model, 416, 100)  # 4 tiles: one full, three partial (letterboxed after the channel is built)
    exp = opl.detect_symbols(img, opl.OracleModel(net, 416, "fp32"), 416, 100)  # channel built by the numpy restatement, forward by torch-CPU
    assert len(exp) > 5
    _same_dets(got, exp, 2e-4, 0.1, "fp32 4-channel detect_symbols 600x740", max_subst=2)


def test_fp32_process_image_on_the_real_sample_file_no_injection(ood, nets, tmp_path):
    """BASELINE configs[0] with nothing injected: process_image(path) on the reference's own Input/Test1.png (9 + 90 tiles, dual scale) in
    fp32 mode against the CPU pipeline running its own fp32 forwards."""
    import os
    from conftest import GOLDEN
    path = os.path.join(GOLDEN, "input", "Test1.png")
    img = ood.detect.imread_bgr(path)
    m128 = ood.model.YOLO(nets[128], imgsz=128, precision="f32")
    m416 = ood.model.YOLO(nets[416], imgsz=416, precision="f32")
    exp, by_scale = opl.process_image(img, [opl.OracleModel(nets[128], 128, "fp32"), opl.OracleModel(nets[416], 416, "fp32")])
    got = ood.detect.process_image(path, str(tmp_path), [m128, m416])
    assert len(exp) > 3
    _same_dets(got, exp, 2e-4, 0.1, "fp32 process_image Test1.png", max_subst=2, max_flips=3)  # ~1900 detections: measured 1 flip


def _match_sets(got, exp, iou_min=0.5):
    """greedy same-class matching by polygon IoU (oracle geometry): -> (matched pairs, unmatched got, unmatched exp)"""
    used, pairs = set(), []
    for gi, g in enumerate(got):
        best, bj = 0.0, -1
        for j, e in enumerate(exp):
            if j in used or e[8] != g[8]:
                continue
            v = og.compute_polygon_iou(list(g[:8]), list(e[:8]))
            if v > best:
                best, bj = v, j
        if bj >= 0 and best >= iou_min:
            used.add(bj)
            pairs.append((gi, bj, best))
    return pairs, len(got) - len(pairs), len(exp) - len(pairs)


@pytest.mark.parametrize("precision,min_frac,max_conf_d,min_mean_iou", [("f16", 0.95, 0.12, 0.97), ("bf16", 0.7, 0.5, 0.85)])
def test_16bit_detection_set_agreement_with_fp32_reference(ood, nets, precision, min_frac, max_conf_d, min_mean_iou):
    """The stated tolerance of the 16-bit forward, end to end and with no injection: detections of the dual-scale pipeline vs the fp32
    reference pipeline.  A 16-bit network flips the few candidates that sit within its logit error of a hard threshold (0.25 / 0.70 /
    NMS 0.7), so agreement is a matched fraction, not identity: fp16 >= 95 % matched (same class, polygon IoU >= 0.5) with |d conf| <= 0.12
    and mean IoU >= 0.97 over the matched pairs (measured on this dense synthetic case, ~600 detections: 97.2 %, 0.078); bf16 (8
    significand bits) is the looser option (78.5 %, 0.35)."""
    img = np.random.default_rng(9).integers(0, 256, (500, 640, 3), dtype=np.uint8)
    m128 = ood.model.YOLO(nets[128], imgsz=128, precision=precision)
    m416 = ood.model.YOLO(nets[416], imgsz=416, precision=precision)
    oms = [opl.OracleModel(nets[128], 128, "fp32"), opl.OracleModel(nets[416], 416, "fp32")]
    exp, _ = opl.process_image(img, oms)
    got = ood.detect.process_image(img, None, [m128, m416])
    pairs, ug, ue = _match_sets(got, exp)
    frac = 2.0 * len(pairs) / max(1, len(got) + len(exp))
    dconf = max((abs(got[i][9] - exp[j][9]) for i, j, _ in pairs), default=0.0)
    ious = [v for _, _, v in pairs]
    print(f"{precision}: {len(got)} vs {len(exp)} detections, matched {len(pairs)} (fraction {frac:.3f}), unmatched {ug}/{ue}, max conf d {dconf:.4f}, "
          f"IoU of matched pairs mean {np.mean(ious):.4f} min {np.min(ious):.3f}")
    assert len(exp) > 3 and frac >= min_frac, frac
    assert dconf <= max_conf_d and np.mean(ious) >= min_mean_iou, (dconf, np.mean(ious))
    # the same agreement split by distance from the confidence thresholds the pipeline applies to a detection (0.25: predictor + consensus
    # low bound, 0.70: consensus high bound, Detect_OBB.py:83, 349-351): a reference detection whose fp32 confidence is at least 0.05 away
    # from both cannot be flipped by the 16-bit confidence error itself -- what remains unmatched there was decided by a NEIGHBOUR's flip
    # (NMS / merge / consensus partner)
    matched_exp = {j for _, j, _ in pairs}
    safe = [j for j, e in enumerate(exp) if min(abs(e[9] - 0.25), abs(e[9] - 0.70)) >= 0.05]
    near = [j for j in range(len(exp)) if j not in set(safe)]
    f_safe = sum(j in matched_exp for j in safe) / max(1, len(safe))
    f_near = sum(j in matched_exp for j in near) / max(1, len(near))
    print(f"{precision}: reference detections >= 0.05 from 0.25 / 0.70: {len(safe)}, matched {f_safe:.4f}; within 0.05: {len(near)}, matched {f_near:.4f}")
    # measured (dense synthetic case): fp16 0.970 / 0.897, bf16 0.817 / 0.513 -- the flips away from the thresholds are second-order: a
    # NEIGHBOUR crossed a threshold and took the detection with it (NMS rival, merge partner, consensus partner)
    assert f_safe >= (0.96 if precision == "f16" else 0.70), f_safe
