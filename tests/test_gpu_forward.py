"""GPU parity of the YOLO11-OBB forward (implicit-GEMM MFMA convs + fused epilogues + attention) vs the torch-CPU oracle.

Two oracles: "bf16" = same graph with the HIP path's rounding points (tight tolerance: only accumulation order and
1-ulp bf16 flips differ) and "fp32" = what the reference computes (stated tolerance of the bf16 arithmetic)."""
import numpy as np
import pytest
import torch

from oracle.yolo11_obb import Yolo11OBB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops as o
    return o


@pytest.fixture(scope="module", params=["f16", "bf16"])
def net_n(ops, request):
    m = Yolo11OBB("n", nc=12, ch=3, seed=0)
    m.prec = request.param
    ops.model_load(m.to_blob(), precision=m.prec)
    return m


def _tiles(seed, B, h, w, ch=3):
    return np.random.default_rng(seed).integers(0, 256, (B, h, w, ch), dtype=np.uint8)


def test_model_info(ops, net_n):
    info = ops.model_info(416, 416)
    assert info == {"nc": 12, "ch": 3, "anchors": 3549, "nconv": 96}
    assert ops.model_info(128, 128)["anchors"] == 336
    ops.forward(torch.as_tensor(_tiles(0, 1, 416, 416)).cuda())  # building a plan synthesises merged records: the blob's count must not change
    assert ops.model_info(416, 416)["nconv"] == 96


ALL_TAPS = ["model.0", "model.1", "model.2.cv1", "model.2.m.0.cv1", "model.2.m.0.cv2", "model.2.cv2", "model.3", "model.4.cv2",
            "model.5", "model.6.cv2", "model.7", "model.8.cv2", "model.9.cv1", "model.9.cv2", "model.10.cv1",
            "model.10.m.0.attn.qkv", "model.10.m.0.attn", "model.10.m.0.attn.pe", "model.10.m.0.ffn.1", "model.10.cv2",
            "model.13.cv2", "model.16.cv2", "model.17", "model.19.cv2", "model.20", "model.22.cv2",
            "model.23.cv2.0.1", "model.23.cv3.0.0.0", "model.23.cv3.0.1.1", "model.23.cv4.2.1"]
def test_layer_taps_match_bf16_oracle(ops, net_n):
    # (statistical, unfused plan only: test_gpu_forward_elems.py checks every element per group of each plan against fp64 bounds)
    x = _tiles(1, 2, 416, 416)
    taps = {}
    net_n.forward_raw(x, net_n.prec, taps)
    ops.model_load(net_n.to_blob(), precision=net_n.prec, tail=False)  # every fusion that swallows an intermediate off: all taps observable
    plan = ops.debug_plan(416, 416)
    assert not any(l.startswith(("bneck ", "c3kimg ", "dwpw ")) or "+model." in l for l in plan), plan
    head = ops.forward(torch.as_tensor(x).cuda())
    torch.cuda.synchronize()
    worst = {}
    for name in ALL_TAPS:
        got = ops.debug_activation(name, 2, 416, 416).cpu()
        exp = taps[name].permute(0, 2, 3, 1)
        if name == "model.10.m.0.attn.qkv":  # device stores [q heads | k heads | v heads]
            nh, kd, hd = 2, 32, 64
            idx = [h * (2 * kd + hd) + d for h in range(nh) for d in range(kd)] + [h * (2 * kd + hd) + kd + d for h in range(nh) for d in range(kd)] + \
                  [h * (2 * kd + hd) + 2 * kd + d for h in range(nh) for d in range(hd)]
            exp = exp[..., idx]
        assert got.shape == exp.shape, name
        if name == "model.10.cv1":  # the b half is updated in place by the PSA block (x = x + attn(x); x = x + ffn(x))
            got, exp = got[..., :128], exp[..., :128]
        d = (got - exp).abs()
        rel = float(d.mean() / exp.abs().mean())
        worst[name] = (round(float(d.max()), 4), round(float(d.mean()), 5), round(rel, 5))
        print(name, worst[name], flush=True)
        # same rounding points on both sides: what remains is fp32 summation order + propagated 1-ulp bf16 flips.
        # A wrong tap/weight/epilogue shows up as O(1) relative error.
        tol = 1.0 if net_n.prec == 'bf16' else 0.3
        assert rel < 5e-2 * tol and float(d.max()) < 1.0 * tol, (name, worst[name])
    ops.model_load(net_n.to_blob(), precision=net_n.prec)


@pytest.mark.parametrize("h,w,B", [(416, 416, 3), (128, 128, 5), (416, 288, 2), (64, 96, 3)])
def test_upsample_concat_read_in_place(ops, net_n, h, w, B):
    """The 1x1 convs behind Upsample + Concat read the low-res tensor and the skip tensor directly: same operands, same k order."""
    x = torch.as_tensor(_tiles(33 + h + w, B, h, w)).cuda()
    ops.model_load(net_n.to_blob(), precision=net_n.prec, upfold=False)
    assert any(l.startswith("upsample") for l in ops.debug_plan(h, w))
    ref = ops.forward(x).clone()
    ref13 = ops.debug_activation("model.13.cv2", B, h, w).clone()
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    assert not any(l.startswith("upsample") for l in ops.debug_plan(h, w))
    got = ops.forward(x)
    got13 = ops.debug_activation("model.13.cv2", B, h, w)
    torch.cuda.synchronize()
    assert float((got13 - ref13).abs().max()) == 0.0
    assert float((got[..., :77] - ref[..., :77]).abs().max()) == 0.0


@pytest.mark.parametrize("h,w,B,ch", [(416, 416, 3, 3), (832, 416, 1, 3), (416, 416, 2, 4)])
def test_front_kernel_matches_separate_launches(ops, h, w, B, ch):
    """model.0 + model.1 + model.2.cv1 in one launch (front.hip, tiles whose sides are multiples of 52) against the stem kernel + the fused
    conv pair: the same k order everywhere; the differences are the accumulators starting at the bias (instead of adding it last) and the
    final rounding of x * sigmoid(x) (one step instead of two), so 16-bit activations flip by an ulp here and there, a flipped stem value
    moves the values behind it by a few ulps, and the head stays within the fused-form tolerance."""
    import make_weights
    blob = open(make_weights.ensure("n", 12, ch, 0), "rb").read()
    x = torch.as_tensor(np.random.default_rng(7 + h + w).integers(0, 256, (B, h, w, ch), dtype=np.uint8)).cuda()
    ops.model_load(blob, precision="f16", front=False)
    assert not any(l.startswith("front") for l in ops.debug_plan(h, w))
    ref_head = ops.forward(x).clone()
    ref = ops.debug_activation("model.2.cv1", B, h, w).clone().float()
    ops.model_load(blob, precision="f16")
    assert any(l.startswith("front model.0+model.1+model.2.cv1") for l in ops.debug_plan(h, w))
    got_head = ops.forward(x)
    got = ops.debug_activation("model.2.cv1", B, h, w).float()
    torch.cuda.synchronize()
    d = (got - ref).abs()
    # 16-bit ulps at the value's binade, with a floor of 2^-2: an output near zero is the 1x1 sum of O(1) inputs that may each have flipped
    ulp = torch.maximum(ref.abs(), torch.tensor(0.25, device="cuda")) * 2.0 ** -10
    print("front vs separate: max ulps", float((d / ulp).max()), "fraction differing", float((d > 0).float().mean()))
    assert float((d / ulp).max()) <= 8.0, float((d / ulp).max())
    assert float((d > 0).float().mean()) < 0.05
    dh = (got_head[..., :65 + 12] - ref_head[..., :65 + 12]).abs()
    assert float(dh.max()) < 0.5 and float(dh.mean()) < 1e-2, (float(dh.max()), float(dh.mean()))


def test_merged_sibling_convs_match_separate_launches(ops, net_n):
    """hmerge: the first convs of the head's box and angle branches read the same feature map; at P5 (one tile per image) they run as one
    80-cout k_conv_igemm launch, at P3 as ONE five-fragment group of k_conv3_pair.  Same k order as the separate launches -> identical."""
    B, h, w = 3, 416, 416
    x = torch.as_tensor(_tiles(19, B, h, w)).cuda()
    ops.model_load(net_n.to_blob(), precision=net_n.prec, hmerge=False)
    assert not any("cv2.0.0|" in l or "cv2.2.0|" in l for l in ops.debug_plan(h, w))
    ref = ops.forward(x).clone()
    ref_a = {n: ops.debug_activation(n, B, h, w).clone() for n in ("model.23.cv2.0.0", "model.23.cv4.0.0", "model.23.cv4.2.0")}
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    plan = ops.debug_plan(h, w)
    assert any("model.23.cv2.0.0|model.23.cv4.0.0" in l and "cout80" in l for l in plan) and any("model.23.cv2.2.0|model.23.cv4.2.0" in l for l in plan), plan
    got = ops.forward(x)
    for n, r in ref_a.items():
        assert torch.equal(ops.debug_activation(n, B, h, w), r), n
    assert torch.equal(got[..., :77], ref[..., :77])


def test_pair_kernel_matches_staged_kernel(ops, net_n):
    """k_conv3_pair (3x3 convs with 64 input channels and 64-cout groups: weights resident in LDS, two half-groups per workgroup, all 64 input
    channels in one k loop, tails straight from registers; stride 1 on 13 x 13 tiles, stride 2 on 4-row stripes) against k_conv_igemm on
    the same layers (four 16-channel stages): the k sums are split differently, so 16-bit values flip by an ulp here and there.  model.4.cv1
    (stride-2 conv + its fused 1x1, identical inputs) is held to 4 ulps; layers further down see propagated flips and are held
    statistically; the fp32 box logits stay within the fused-form tolerance."""
    B, h, w = 3, 416, 416
    x = torch.as_tensor(_tiles(77, B, h, w)).cuda()
    names = ("model.4.cv1", "model.17", "model.23.cv2.0.0")
    ops.model_load(net_n.to_blob(), precision=net_n.prec, pair=False)
    assert not any("CK64" in l and ("cv2.0.0" in l or "model.3+" in l) for l in ops.debug_plan(h, w))
    ref_head = ops.forward(x).clone()
    ref = {n: ops.debug_activation(n, B, h, w).clone().float() for n in names}
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    plan = ops.debug_plan(h, w)
    assert any("CK64" in l and "cv2.0.0" in l for l in plan) and any("model.3+model.4.cv1" in l and "TH4" in l for l in plan) and any("model.17" in l and "TH4" in l for l in plan), plan
    head = ops.forward(x)
    u = 2.0 ** -10 if net_n.prec == "f16" else 2.0 ** -7
    for n in names:
        got = ops.debug_activation(n, B, h, w).float()
        d = (got - ref[n]).abs()
        ulps = d / (u * torch.maximum(ref[n].abs(), torch.tensor(0.25, device="cuda")))
        print(n, "max ulps", float(ulps.max()), "fraction differing", float((d > 0).float().mean()), "mean |d|", float(d.mean()))
        if n == "model.4.cv1":
            assert float(ulps.max()) <= 4.0 and float((d > 0).float().mean()) < 0.05  # (a flipped conv output moves the 1x1 behind it by another ulp or two)
        else:
            assert float(d.mean()) < (5e-3 if net_n.prec == "f16" else 5e-2) and float(d.max()) < (0.25 if net_n.prec == "f16" else 1.5)
    dh = (head[..., :77] - ref_head[..., :77]).abs()
    assert float(dh.max()) < (0.3 if net_n.prec == "f16" else 2.0) and float(dh.mean()) < (3e-3 if net_n.prec == "f16" else 3e-2), (float(dh.max()), float(dh.mean()))


@pytest.mark.parametrize("h,w,B", [(128, 128, 5), (128, 128, 1030), (64, 64, 37), (128, 64, 6)])
def test_multi_image_tiles_are_bit_identical(ops, net_n, h, w, B):
    """`nitile`: the 3x3 convs on 4 x 4 / 2 x 2 maps take several whole images per 64-pixel tile (k_conv_igemm NIT) instead of one image
    padded to an 8 x 8 tile -- same operands, same k order, so the head must agree BIT FOR BIT; batch sizes that leave the last tile partly
    empty, a batch above one round and a non-square tile (no 4 x 4 / 2 x 2 level of its own shape: plan unchanged) included."""
    x = torch.as_tensor(_tiles(5 + h + B, B, h, w)).cuda()
    ops.model_load(net_n.to_blob(), precision=net_n.prec, nitile=False)
    assert not any(" NI4 " in l or " NI16 " in l for l in ops.debug_plan(h, w))
    one = ops.forward(x).clone()
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    plan = ops.debug_plan(h, w)
    if h == w:
        assert any(" NI4 " in l for l in plan), plan
    ni = ops.forward(x)
    assert torch.equal(one[..., :77], ni[..., :77]), float((one - ni)[..., :77].abs().max())


@pytest.mark.parametrize("h,w,B", [(416, 416, 3), (128, 128, 5), (416, 288, 2), (192, 416, 2), (64, 96, 3)])
def test_tail_fusion_matches_separate_launches(ops, net_n, h, w, B):
    """The fused trailing 1x1 reads the producer's 16-bit output from LDS instead of HBM: same values, same k order -> identical head."""
    x = torch.as_tensor(_tiles(55 + h + w, B, h, w)).cuda()
    # (the fused Bottleneck and the per-image C3k kernel sum their k in one channel stage where the separate kernels use several:
    #  1-ulp flips, tested below -- both stay off on both sides here)
    ops.model_load(net_n.to_blob(), precision=net_n.prec, tail=False)
    ref = ops.forward(x).clone()
    # (front: the one-launch model.0 + model.1 + model.2.cv1 rounds x * sigmoid(x) to 16 bit in one step (v_fma_mixlo_f16) where the separate
    #  kernels round to fp32 first: 1-ulp flips, tested in test_front_kernel_matches_separate_launches)
    ops.model_load(net_n.to_blob(), precision=net_n.prec, tail=True, bneck=False, c3kimg=False, front=False)
    if (h, w) == (416, 416):
        assert any("+model.23.cv2.0.2" in l for l in ops.debug_plan(h, w))
    got = ops.forward(x)
    torch.cuda.synchronize()
    d = (got[..., :77] - ref[..., :77]).abs()
    assert float(d.max()) <= 1e-5, float(d.max())


def test_concurrent_chains_and_rounds_match_small_batches(ops, net_n):
    """A large batch is walked in rounds, each issued as two concurrent half-batch chains that address their own image range of every
    activation buffer (plain, channel-blocked and virtual-concat ones alike): the result must equal the same tiles run in small calls."""
    B = 1100  # rounds of 1024 + 76 tiles, both split into two chains
    x = torch.as_tensor(_tiles(5, B, 128, 128)).cuda()
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    big = ops.forward(x).clone()
    big2 = ops.forward(x).clone()          # second call: hipGraph replay of the captured round
    small = torch.cat([ops.forward(x[i:i + 50].contiguous()).clone() for i in range(0, B, 50)])
    torch.cuda.synchronize()
    assert torch.equal(big, small) and torch.equal(big2, small)


@pytest.mark.parametrize("B", [5, 65, 300])
def test_head_of_a_tile_does_not_depend_on_its_batch(ops, net_n, B):
    """416-px tiles through the persistent kernels (k_front, k_conv3_pair: tiles dealt to workgroups and half-groups by index, odd counts,
    one- and two-chain rounds): every tile's head must equal the head of that tile run alone, and a replay must reproduce it."""
    x = torch.as_tensor(_tiles(B, B, 416, 416)).cuda()
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    got = ops.forward(x).clone()
    again = ops.forward(x).clone()
    for k in sorted({0, 1 % B, B // 2, B - 2, B - 1}):
        assert torch.equal(ops.forward(x[k:k + 1].contiguous())[0], got[k]), k
    assert torch.equal(got, again)


@pytest.mark.parametrize("h,w,B", [(416, 416, 3), (416, 288, 2), (128, 128, 4)])
def test_cv1_behind_stride2_conv(ops, net_n, h, w, B):
    """model.1 / model.3 (3x3 stride 2) run the cv1 of the following C3k2 block on their staged output tile (their own output tensor
    is never written): same 16-bit rounding of the intermediate, same k order -> identical activations and head."""
    x = torch.as_tensor(_tiles(23 + h, B, h, w)).cuda()
    ops.model_load(net_n.to_blob(), precision=net_n.prec, tail16=False, pair=False)
    assert not any("+model.2.cv1" in l for l in ops.debug_plan(h, w))
    ref_head = ops.forward(x).clone()
    ref = {n: ops.debug_activation(n, B, h, w).clone() for n in ("model.2.cv1", "model.4.cv1")}
    ops.model_load(net_n.to_blob(), precision=net_n.prec, front=False, pair=False)  # (front and the pair kernel have their own tests: different rounding points / k order)
    plan = ops.debug_plan(h, w)
    fused = [l for l in plan if "model.1+model.2.cv1" in l or "model.3+model.4.cv1" in l]
    assert len(fused) == (2 if (h, w) == (416, 416) else 0), plan   # 13x13 output tiles only (every level of a full 416-px tile)
    head = ops.forward(x)
    for n, r in ref.items():
        assert torch.equal(ops.debug_activation(n, B, h, w), r), n
    assert torch.equal(head[..., :77], ref_head[..., :77])


@pytest.mark.parametrize("h,w,B", [(416, 416, 3), (128, 128, 9)])
def test_depthwise_pointwise_stripes(ops, net_n, h, w, B):
    """Class branch of the head at the 52 / 26 levels (416-px tiles) and the 16 / 8 levels (128-px tiles): DWConv 3x3 -> Conv 1x1 (-> plain 1x1
    into the head tensor) as one stripe kernel per pair, the depthwise result living only in registers as the MFMA operand.  Same arithmetic
    and rounding points as the separate kernels for the first pair (identical activations); the trailing 1x1 sums its 64 inputs in a
    different k order (fp32: ~1e-6)."""
    x = torch.as_tensor(_tiles(71, B, h, w)).cuda()
    names = ("model.23.cv3.0.0.1", "model.23.cv3.1.0.1")
    ops.model_load(net_n.to_blob(), precision=net_n.prec, dwpw=False)
    assert not any(l.startswith("dwpw ") for l in ops.debug_plan(h, w))
    head_ref = ops.forward(x).clone()
    ref = {n: ops.debug_activation(n, B, h, w).clone() for n in names}
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    plan = ops.debug_plan(h, w)
    assert sum(l.startswith("dwpw ") for l in plan) == 4, plan
    assert sum(l.startswith("dwconv model.23.cv3.") for l in plan) == 2, plan   # the 13x13 level keeps the separate kernels
    head = ops.forward(x)
    for n in names:
        assert torch.equal(ops.debug_activation(n, B, h, w), ref[n]), n
    d = (head[..., :77] - head_ref[..., :77]).abs()
    assert float(d[..., :64].max()) == 0.0 and float(d[..., 76].max()) == 0.0   # box and angle branches untouched
    print("class logits: max diff", float(d[..., 64:76].max()))
    assert float(d[..., 64:76].max()) <= 2e-5


def test_c3k_image_kernel(ops, net_n):
    """Inner C3k of the stride-32 level as one persistent workgroup per image (c3kimg.hip) vs the same block as separate launches
    (identical inputs: only this block's implementation differs).  Same rounding points; the 3x3 convs sum all 64 input channels in one
    k loop instead of four channel stages -> rare 1-ulp flips that propagate through the block's six layers."""
    B, h, w = 3, 416, 416
    x = torch.as_tensor(_tiles(17, B, h, w)).cuda()
    ops.model_load(net_n.to_blob(), precision=net_n.prec, c3kimg=False)
    assert not any(l.startswith("c3kimg ") for l in ops.debug_plan(h, w))
    ops.forward(x)
    ref = {n: ops.debug_activation(n, B, h, w).clone() for n in ("model.8.m.0.cv3", "model.8.cv2")}
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    assert sum(l.startswith("c3kimg ") for l in ops.debug_plan(h, w)) == 2
    ops.forward(x)
    for n, r in ref.items():
        d = (ops.debug_activation(n, B, h, w) - r).abs()
        print(n, float(d.max()), float(d.mean()), float(r.abs().mean()))
        assert float(d.mean()) < (1e-3 if net_n.prec == "f16" else 1e-2) and float(d.max()) < (0.05 if net_n.prec == "f16" else 0.4)


@pytest.mark.parametrize("h,w,B", [(416, 416, 3), (128, 128, 9)])
def test_fused_bottleneck_stripes(ops, net_n, h, w, B):
    """Bottleneck(3x3, 3x3, shortcut) of the 104 / 52 levels (416-px tiles) and of the 32 / 16 levels (128-px tiles: the dual-scale default) as
    one stripe kernel: same rounding points as the two separate convs.  The 16 -> 8 -> 16 block also sums in the same order (bit-identical);
    the 32 -> 16 -> 32 block sums all 32 input channels in one k loop where the separate kernel uses two channel stages: rare 1-ulp flips of
    16-bit values."""
    x = torch.as_tensor(_tiles(91, B, h, w)).cuda()
    ref = {}
    ops.model_load(net_n.to_blob(), precision=net_n.prec, tail=False)
    head_ref = ops.forward(x).clone()
    for name in ("model.2.m.0.cv2", "model.4.m.0.cv2", "model.16.m.0.cv2"):
        ref[name] = ops.debug_activation(name, B, h, w).clone()
    # keep y2 observable: the closing 1x1 as its own launch (fused form: next test); front off: the reference side (tail=False) has no one-launch front
    ops.model_load(net_n.to_blob(), precision=net_n.prec, bneck_cv2=False, front=False)
    plan = ops.debug_plan(h, w)
    assert sum(l.startswith("bneck ") for l in plan) == 3, plan
    head = ops.forward(x)
    ulp = 2.0 ** -10 if net_n.prec == "f16" else 2.0 ** -7
    for name in ref:
        got = ops.debug_activation(name, B, h, w)
        d = (got - ref[name]).abs()
        print(name, float(d.max()), float((d > 0).float().mean()))
        if name == "model.2.m.0.cv2":
            assert float(d.max()) == 0.0
        elif name == "model.16.m.0.cv2":  # its INPUT already carries the propagated flips of model.4: statistical closeness only
            assert float(d.mean()) < (5e-3 if net_n.prec == "f16" else 5e-2) and float(d.max()) < (0.25 if net_n.prec == "f16" else 1.5)
        else:
            assert float((d / ref[name].abs().clamp_min(1.0)).max()) <= 4 * ulp and float((d > 0).float().mean()) < 0.05
    dh = (head[..., :77] - head_ref[..., :77]).abs()
    # (128-px tiles: the same 1-ulp flips reach a head of 336 anchors through 4 x 4 / 8 x 8 maps -- measured 4.7e-3 for fp16)
    assert float(dh.mean()) < (3e-3 if net_n.prec == "f16" else 3e-2) * (1 if h == 416 else 2.5), float(dh.mean())


@pytest.mark.parametrize("h,w,B", [(416, 416, 3), (128, 128, 9)])
def test_closing_1x1_behind_the_bottleneck(ops, net_n, h, w, B):
    """C3k2 blocks 2, 4 and 16: cv2 over [y0 | y1 | y2] runs on every 16-pixel fragment right behind the Bottleneck's second conv
    (y0 from global memory, y1 from the LDS image, y2 from the producing lane's registers).  Same 16-bit rounding of y2; the k sum is
    split differently from the stand-alone 1x1 (and uses a 16-wide MFMA step for the 16-channel block): 1-ulp flips of 16-bit outputs."""
    x = torch.as_tensor(_tiles(37, B, h, w)).cuda()
    names = ("model.2.cv2", "model.4.cv2", "model.16.cv2")
    ops.model_load(net_n.to_blob(), precision=net_n.prec, bneck_cv2=False)
    assert not any(l.startswith("bneck ") and "+model." in l for l in ops.debug_plan(h, w))
    head_ref = ops.forward(x).clone()
    ref = {n: ops.debug_activation(n, B, h, w).clone() for n in names}
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    plan = ops.debug_plan(h, w)
    assert sum(l.startswith("bneck ") and ".m.0+model." in l for l in plan) == 3, plan
    assert not any(l.startswith("conv model.2.cv2 ") or l.startswith("conv model.4.cv2 ") or l.startswith("conv model.16.cv2 ") for l in plan)
    head = ops.forward(x)
    ulp = 2.0 ** -10 if net_n.prec == "f16" else 2.0 ** -7
    for n in names:
        got = ops.debug_activation(n, B, h, w)
        assert got.shape == ref[n].shape
        d = (got - ref[n]).abs()
        print(n, tuple(got.shape), float(d.max()), float((d > 0).float().mean()))
        if n == "model.16.cv2":  # its input already carries the propagated flips of the earlier blocks
            assert float(d.mean()) < (5e-3 if net_n.prec == "f16" else 5e-2) and float(d.max()) < (0.25 if net_n.prec == "f16" else 1.5)
        else:
            # (model.4 sees model.2's few flipped inputs on top of its own)
            assert float((d / ref[n].abs().clamp_min(1.0)).max()) <= 4 * ulp and float((d > 0).float().mean()) < (0.01 if n == "model.2.cv2" else 0.15)
    dh = (head[..., :77] - head_ref[..., :77]).abs()
    # (128-px tiles: measured 5.4e-3 for fp16 -- see test_fused_bottleneck_stripes)
    assert float(dh.mean()) < (3e-3 if net_n.prec == "f16" else 3e-2) * (1 if h == 416 else 2.5), float(dh.mean())


@pytest.mark.parametrize("h,w,B", [(416, 416, 3), (128, 128, 5), (416, 288, 1), (192, 416, 2)])
def test_head_matches_oracles(ops, net_n, h, w, B):
    ops.model_load(net_n.to_blob(), precision=net_n.prec)  # explicitly: the default options, whatever the previous test left loaded
    x = _tiles(10 + h + w, B, h, w)
    head = ops.forward(torch.as_tensor(x).cuda()).cpu()[..., :77]
    ref16 = net_n.forward_raw(x, net_n.prec)
    ref32 = net_n.forward_raw(x, "fp32")
    assert head.shape == ref16.shape
    d16 = (head - ref16).abs()
    d32 = (head - ref32).abs()
    b32 = (ref16 - ref32).abs()
    print(net_n.prec, h, w, "vs 16-bit oracle max/mean", float(d16.max()), float(d16.mean()), "vs fp32", float(d32.max()), float(d32.mean()),
          "oracle bf16-vs-fp32", float(b32.max()), float(b32.mean()))
    # same arithmetic model: only fp32 summation order + rare 16-bit 1-ulp flips propagate.  Bounds = the largest value measured over the four
    # shapes (round 4: f16 max 0.182 / mean 0.0062, bf16 max 1.205 / mean 0.036) + 50 %
    mx16, mean16 = (1.81, 0.054) if net_n.prec == 'bf16' else (0.28, 0.0093)
    assert float(d16.mean()) < mean16 and float(d16.max()) < mx16
    # against the reference's fp32 arithmetic the HIP path is as close as the bf16 model itself (stated tolerance)
    assert float(d32.mean()) < 1.5 * float(b32.mean()) + 1e-3
    conf16 = torch.sigmoid(ref32[..., 64:76]).amax(-1)
    confg = torch.sigmoid(head[..., 64:76]).amax(-1)
    dc = (conf16 - confg).abs()
    print('conf |d| max/mean', float(dc.max()), float(dc.mean()))
    cmx, cmean = (0.61, 0.024) if net_n.prec == 'bf16' else (0.086, 0.0026)  # measured 0.406 / 0.0158 (bf16), 0.057 / 0.0017 (f16), + 50 %
    assert float(dc.mean()) < cmean and float(dc.max()) < cmx


def test_forward_is_deterministic_and_batch_invariant(ops, net_n):
    x = _tiles(3, 4, 416, 416)
    t = torch.as_tensor(x).cuda()
    a = ops.forward(t)
    b = ops.forward(t)
    assert torch.equal(a, b)
    c = ops.forward(t[1:3].contiguous())
    assert torch.equal(a[1:3], c)  # a tile's result does not depend on its neighbours in the batch


def test_four_channel_and_s_scale_models(ops):
    """config 4 network input (RGB + DT-edge: 4 channels, no BGR flip) and the wider 's' scale run through the same kernels."""
    for scale, ch, h, w in (("n", 4, 416, 416), ("s", 3, 128, 160)):
        m = Yolo11OBB(scale, nc=12, ch=ch, seed=3)
        ops.model_load(m.to_blob())
        x = np.random.default_rng(7).integers(0, 256, (2, h, w, ch), dtype=np.uint8)
        head = ops.forward(torch.as_tensor(x).cuda()).cpu()[..., :77]
        r16, r32 = m.forward_raw(x, "f16"), m.forward_raw(x, "fp32")
        d16, d32, b32 = (head - r16).abs(), (head - r32).abs(), (r16 - r32).abs()
        print(scale, ch, "vs f16 oracle", float(d16.max()), float(d16.mean()), "vs fp32", float(d32.mean()), "oracle f16-vs-fp32", float(b32.mean()))
        assert float(d16.mean()) < 0.02 and float(d16.max()) < 1.0
        assert float(d32.mean()) < 1.5 * float(b32.mean()) + 1e-3


def test_hipgraph_capture_and_replay(ops, net_n):
    """The path that produces the headline number: on a non-default stream the second sighting of (batch, input, output) is captured
    into a hipGraph (two half-batch chains forked onto side streams inside the capture for B >= 64) and later calls replay it.  Replays
    must equal the eager result on the null stream (where capture is impossible), bit for bit; graph = 0 must give the same again."""
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    for B, h, w in ((96, 128, 128), (3, 416, 416)):
        x = torch.as_tensor(_tiles(41 + B, B, h, w)).cuda()
        eager = ops.forward(x).clone()           # null stream: hipStreamBeginCapture fails there -> eager launches
        buf = torch.zeros_like(eager)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            outs = []
            for _ in range(4):                   # 1st eager, 2nd captured + launched, 3rd / 4th replayed
                buf.zero_()
                ops.forward(x, out=buf)
                outs.append(buf.clone())
        st.synchronize()
        for o in outs:
            assert torch.equal(o, eager), (B, h, w)
        ops._call("obb_set_option", ops.ctx(), b"graph", 0)
        try:
            with torch.cuda.stream(st):
                ops.forward(x, out=buf)
            st.synchronize()
            assert torch.equal(buf, eager)
        finally:
            ops._call("obb_set_option", ops.ctx(), b"graph", 1)


def test_registered_ops_and_torch_cuda_graph(ops, net_n):
    """The C-ABI is registered with the torch dispatcher (torch.ops.obbhip.*): call it directly, and capture forward + decode_nms of
    the registered ops in a torch.cuda.CUDAGraph (the library's launches join the caller's capture), then replay on new input bytes."""
    ops.model_load(net_n.to_blob(), precision=net_n.prec)
    assert "obbhip::forward" in str(torch.ops.obbhip.forward.default._schema)
    B, h, w = 2, 128, 128
    x = torch.as_tensor(_tiles(3, B, h, w)).cuda()
    ref_head = ops.forward(x).clone()
    ref_det, ref_cnt = ops.decode_nms(ref_head, h, w, 0.25, 0.7, 300)
    head = torch.zeros_like(ref_head)
    torch.ops.obbhip.forward(x, head)                       # straight through the dispatcher
    assert torch.equal(head, ref_head)
    with pytest.raises(Exception):
        torch.ops.obbhip.forward(x.cpu(), head.cpu())       # no CPU implementation is registered
    det, cnt = torch.zeros_like(ref_det), torch.zeros_like(ref_cnt)
    xin = x.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.ops.obbhip.forward(xin, head)                 # warm-up on the side stream (plans, slabs, workspaces exist before capture)
        torch.ops.obbhip.decode_nms(head, h, w, 0.25, 0.7, 300, det, cnt)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        torch.ops.obbhip.forward(xin, head)
        torch.ops.obbhip.decode_nms(head, h, w, 0.25, 0.7, 300, det, cnt)
    x2 = torch.as_tensor(_tiles(4, B, h, w)).cuda()
    xin.copy_(x2)
    head.zero_(); det.zero_(); cnt.zero_()
    g.replay()
    torch.cuda.synchronize()
    exp_head = ops.forward(x2)
    exp_det, exp_cnt = ops.decode_nms(exp_head, h, w, 0.25, 0.7, 300)
    assert torch.equal(head, exp_head) and torch.equal(cnt, exp_cnt) and torch.equal(det, exp_det)
    # obb_merge_detections has no host read at any n (the sparse / dense decision is taken on the device): captured at three sizes -- the
    # LDS-resident segment kernel, the all-pairs edge list, the grid pair search -- and replayed on new boxes
    import synth
    for n in (300, 2000, 9000):
        b1, c1, s1, _ = synth.make_dets(n, n, extent=60.0 * n ** 0.5)
        b2, c2, s2, _ = synth.make_dets(n + 1, n, extent=60.0 * n ** 0.5)
        Bt, Ct, St = torch.tensor(b1).cuda(), torch.tensor(c1).cuda(), torch.tensor(s1).cuda()
        order, keep, nk = ops.merge_detections(Bt, Ct, St, 0.4)  # eager first: workspaces and function attributes exist before the capture
        gm = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gm):
            torch.ops.obbhip.merge_detections(Bt, Ct, St, 0.4, order, keep, nk)
        Bt.copy_(torch.tensor(b2)); Ct.copy_(torch.tensor(c2)); St.copy_(torch.tensor(s2))
        order.zero_(); keep.zero_(); nk.zero_()
        gm.replay()
        torch.cuda.synchronize()
        eo, ek, enk = ops.merge_detections(Bt, Ct, St, 0.4)
        assert torch.equal(order, eo) and torch.equal(keep, ek) and torch.equal(nk, enk) and 0 < int(nk.item()) < n, n


def test_model_slots_are_released(ops):
    """YOLO.close() hands the model slot (weights, slabs, graphs) back: far more than 64 constructions work in one process."""
    from oriented_object_detection_amd.model import YOLO
    m = Yolo11OBB("n", nc=12, ch=3, seed=5)
    blob = m.to_blob()
    x = torch.as_tensor(_tiles(1, 1, 64, 64)).cuda()
    first = None
    for i in range(70):
        y = YOLO(blob, imgsz=64)
        y._ensure_active()
        out = ops.forward(x).clone()
        first = out if first is None else first
        assert torch.equal(out, first)
        y.close()
    with pytest.raises(RuntimeError):
        y._ensure_active()
