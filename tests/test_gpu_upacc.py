"""`upacc` (fp32): the two 1x1 convs behind [Upsample x2 | skip] (model.13.cv1, model.16.cv1) as two launches each -- the product over the
upsampled channels once per COARSE pixel (k_pw_f32, raw accumulators), then the skip channels at full resolution with the accumulators
starting from it (k_conv_f32 AINIT).  The exact-f32 MFMA is a k-ordered fma chain and the one-launch form runs the upsampled channels first,
into zeroed accumulators, so both forms compute the same chain: every tensor must agree BIT FOR BIT, and the plan must count 3/4 of the
upsampled half's multiply-adds less."""
import numpy as np
import pytest
import torch

from oracle.yolo11_obb import Yolo11OBB

pytestmark = pytest.mark.gpu

LAYERS = (("model.13.cv1", "model.10.cv2", 16), ("model.16.cv1", "model.13.cv2", 8))  # (layer, producer of the upsampled member, stride)
NAMES = ("model.13.cv1", "model.16.cv1", "x13", "x16", "model.13.cv2", "model.16.cv2")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    return ops


@pytest.fixture(scope="module")
def nets():
    return {"n": Yolo11OBB("n", nc=12, ch=3, seed=0), "s": Yolo11OBB("s", nc=12, ch=3, seed=2)}


def _tiles(seed, B, h, w):
    return torch.as_tensor(np.random.default_rng(seed).integers(0, 256, (B, h, w, 3), dtype=np.uint8)).cuda()


def _total_macs(plan):
    return int([l for l in plan if l.startswith("total_macs")][0].split()[1])


def _saved_macs(net, h, w):
    return sum((h // s) * (w // s) * net.convs[name].c2 * net.convs[prod].c2 * 3 // 4 for name, prod, s in LAYERS)


@pytest.mark.parametrize("h,w,B,scale", [(64, 64, 3, "n"), (64, 96, 3, "n"), (416, 288, 2, "n"), (128, 128, 65, "n"), (64, 96, 2, "s")])
def test_upacc_is_bit_identical_to_the_one_launch_form(ops, nets, h, w, B, scale):
    net = nets[scale]
    x = _tiles(41 + h + w + B, B, h, w)
    out = None
    res = {}
    for key, kw in (("off", dict(upacc=False)), ("on", {})):
        ops.model_load(net.to_blob(), precision="f32", **kw)
        plan = ops.debug_plan(h, w)
        n_acc, n_up, n_vcat = sum(" upacc1 " in l for l in plan), sum(".up " in l for l in plan), sum(" vcat1 " in l for l in plan)
        assert (n_acc, n_up, n_vcat) == ((2, 2, 2) if key == "on" else (0, 0, 2)), plan
        out = torch.zeros_like(ops.forward(x))  # (a head tensor of our own: stable addresses, so that the library captures and replays)
        heads = [ops.forward(x, out=out)[..., :77].clone() for _ in range(3)]  # eager, captured, replayed: two chains at B >= 64
        for i, t in enumerate(heads[1:]):
            assert torch.equal(heads[0], t), (key, i + 1, float((heads[0] - t).abs().max()))
        res[key] = (_total_macs(plan), heads[0].cpu(), {n: ops.debug_activation(n, B, h, w).cpu() for n in NAMES})
    assert res["off"][0] - res["on"][0] == _saved_macs(net, h, w), (res["off"][0], res["on"][0], _saved_macs(net, h, w))
    assert torch.equal(res["off"][1], res["on"][1]), float((res["off"][1] - res["on"][1]).abs().max())
    for n in NAMES:
        assert torch.equal(res["off"][2][n], res["on"][2][n]), n


def test_upacc_equals_the_materialised_upsample_and_concat(ops, nets):
    """against the one-kernel-per-layer plan (Upsample and Concat written to memory), not only against the form it replaces"""
    net, (h, w, B) = nets["n"], (64, 96, 3)
    x = _tiles(5, B, h, w)
    ops.model_load(net.to_blob(), precision="f32", tail=False, upfold=False, sppf_fuse=False, stem=False)
    assert not any(" vcat1 " in l or " upacc1 " in l for l in ops.debug_plan(h, w))
    plain = ops.forward(x).cpu()
    taps = {n: ops.debug_activation(n, B, h, w).cpu() for n in NAMES}
    ops.model_load(net.to_blob(), precision="f32", stem=False)  # (the row-stripe input layer sums in another order: off on both sides)
    assert sum(" upacc1 " in l for l in ops.debug_plan(h, w)) == 2
    fused = ops.forward(x).cpu()
    assert torch.equal(plain[..., :77], fused[..., :77]), float((plain - fused)[..., :77].abs().max())
    for n, t in taps.items():
        assert torch.equal(t, ops.debug_activation(n, B, h, w).cpu()), n


def test_upacc_needs_upfold(ops, nets):
    net = nets["n"]
    ops.model_load(net.to_blob(), precision="f32", upfold=False)
    a = ops.debug_plan(64, 96)
    ops.model_load(net.to_blob(), precision="f32", upfold=False, upacc=True)
    assert ops.debug_plan(64, 96) == a and not any(" upacc1 " in l or ".up " in l for l in a)
    ops.model_load(net.to_blob(), precision="f32", upfold=False, upacc=False)
    assert ops.debug_plan(64, 96) == a
