"""CPU checks of the narrow-channel slice (csrc/narrowgrad.hip: the head's 1x1 + bias outputs, the stem on the uint8 tile): the fp64 references of
tests/narrow_ref.py against torch.autograd, `train.train_kernel_of` on every conv of YOLO11-OBB n / s, the launchers' own work splits through the
host-only geometry entry points, the argument checks of the new ops, and the rounded-against-plain measurement that sets the tolerances of the
assembled GPU tests.  No GPU."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import narrow_ref as NR
import train_shapes as TS
from oracle.yolo11_obb import Yolo11OBB


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _pkg():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    import oriented_object_detection_amd.train as TR
    return _lib, ops, TR


# ---------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("B,H,W,cin,cout", [(2, 7, 5, 16, 3), (1, 1, 1, 8, 1), (2, 3, 4, 8, 17)])
def test_head_references_equal_autograd(B, H, W, cin, cout):
    g = torch.Generator().manual_seed(H * 10 + W + cout)
    x = torch.randn(B, H, W, cin, generator=g, dtype=torch.float64)
    dy = torch.randn(B, H, W, cout, generator=g, dtype=torch.float64)
    w, b = torch.randn(cout, cin, generator=g, dtype=torch.float64), torch.randn(cout, generator=g, dtype=torch.float64)
    xr, wr, br = _nchw(x).clone().requires_grad_(True), w.view(cout, cin, 1, 1).clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br)
    y.backward(_nchw(dy))
    dx, dw, db = NR.head_bwd_ref(x, dy, w)
    for name, got, ref in (("y", _nchw(NR.head_fwd_ref(x, w, b)), y.detach()), ("dx", _nchw(dx), xr.grad), ("dw", dw, wr.grad.view(cout, cin)), ("db", db, br.grad)):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name


@pytest.mark.parametrize("B,H,W,cin,cout", [(2, 7, 5, 3, 8), (1, 1, 1, 3, 8), (2, 2, 1, 4, 16), (1, 8, 6, 4, 8)])
def test_stem_references_equal_autograd(B, H, W, cin, cout):
    g = torch.Generator().manual_seed(H * 10 + W + cin)
    x = torch.randint(0, 256, (B, H, W, cin), generator=g, dtype=torch.uint8)
    xq = NR.stem_operand(x)
    assert torch.equal(xq, NR.bf16(x.double() / 255.0)), "bf16(fp32(v / 255)) differs from bf16(v / 255) for some byte"
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    z = F.conv2d(_nchw(xq), w, stride=2, padding=1)
    dz = torch.randn(B, (H + 1) // 2, (W + 1) // 2, cout, generator=g, dtype=torch.float64)
    z.backward(_nchw(dz))
    for name, got, ref in (("z", _nchw(NR.stem_fwd_ref(xq, w.detach())), z.detach()), ("dw", NR.stem_wgrad_ref(xq, dz), w.grad)):
        assert tuple(got.shape) == tuple(ref.shape) and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name


def test_stem_operand_of_every_byte():
    """bf16(v / 255): the fp32 quotient and the fp64 quotient round to the same bf16 value for all 256 bytes, 0 -> 0 and 255 -> 1 exactly."""
    v = torch.arange(256, dtype=torch.uint8)
    q = NR.stem_operand(v)
    assert torch.equal(q, NR.bf16(v.double() / 255.0)) and float(q[0]) == 0.0 and float(q[255]) == 1.0


# ---------------------------------------------------------------------------------------------- train_kernel_of
@pytest.mark.parametrize("scale", ["n", "s"])
@pytest.mark.parametrize("ch", [3, 4])
def test_every_conv_of_the_model_has_a_training_kernel(scale, ch):
    """Every conv of Yolo11OBB(scale) at nc = 12 gets a route, and exactly the layers train_shapes.conv_class calls GAP with g = 1 are the stem and
    the narrow head outputs."""
    _, _, TR = _pkg()
    m = Yolo11OBB(scale, nc=12, ch=ch, seed=0)
    routes = {}
    for name, r in m.convs.items():
        routes[name] = TR.train_kernel_of(r.k, r.s, r.g, r.c1, r.c2)
        gap = TS.conv_class(r.k, r.s, r.g, r.c1, r.c2) == TS.GAP
        if r.g != 1:
            assert routes[name] == "depthwise", (name, routes[name])
        elif gap:
            assert routes[name] in ("stem", "head_out"), (name, routes[name])
            assert routes[name] == ("stem" if name.startswith("model.0.") or name == "model.0" else "head_out"), (name, routes[name])
        else:
            assert routes[name] == "dense", (name, routes[name])
    kinds = set(routes.values())
    assert kinds == {"dense", "depthwise", "stem", "head_out"}, kinds
    assert sum(v == "stem" for v in routes.values()) == 1
    assert sum(v == "head_out" for v in routes.values()) == 6  # cv3.i.2 (nc = 12) and cv4.i.2 (1) on three levels; cv2.i.2 has 64 outputs: dense


def test_train_kernel_of_refusals():
    _, _, TR = _pkg()
    for bad in ((3, 2, 1, 5, 16), (3, 1, 1, 64, 12), (1, 1, 1, 64, 65), (3, 1, 1, 3, 16), (1, 1, 1, 12, 12), (3, 1, 2, 64, 64), (1, 1, 1, 520, 12)):
        with pytest.raises(ValueError):
            TR.train_kernel_of(*bad)
    assert TR.train_kernel_of(1, 1, 1, 64, 12) == "head_out" and TR.train_kernel_of(1, 1, 1, 16, 1) == "head_out"
    assert TR.train_kernel_of(3, 2, 1, 4, 32) == "stem" and TR.train_kernel_of(1, 1, 1, 64, 64) == "dense" and TR.train_kernel_of(3, 1, 64, 64, 64) == "depthwise"
    with pytest.raises(ValueError):  # wgrad_route keeps refusing what is no multiple of 8
        TR.wgrad_route(64, 12)


# ---------------------------------------------------------------------------------------------- geometry
def _depth(rp):
    return max(0, math.ceil(math.log2(rp)))


@pytest.mark.parametrize("B,H,W,cin,cout", NR.HEAD_SHAPES + [(16, 52, 52, 64, 12), (16, 52, 52, 16, 1), (64, 104, 104, 512, 64)])
def test_head_bwd_geometry(B, H, W, cin, cout):
    """L is the chain of the reported split (lane run + LDS tree depth + 64 strided walkers + their tree of 6), the lanes cover every pixel."""
    _, ops, _ = _pkg()
    N = B * H * W
    run, RP, nbx, L = ops.headconv_bwd_geometry(N, cin, cout)
    assert (run, RP, nbx, L) == ops.headconv_bwd_geometry(N, cin, cout)
    assert run >= 1 and 1 <= RP <= 256 and 1 <= nbx <= 512
    assert L == run + _depth(RP) + -(-nbx // 64) + 6, (run, RP, nbx, L)
    assert run * nbx * RP >= N > (run - 1) * nbx * RP, (run, RP, nbx, N)
    if (B, H, W) != (64, 104, 104):
        assert L <= 64, L


@pytest.mark.parametrize("B,H,W,cin,cout", NR.STEM_SHAPES + [(16, 416, 416, 3, 16), (16, 416, 416, 4, 32)])
def test_stem_wgrad_geometry(B, H, W, cin, cout):
    _, ops, _ = _pkg()
    NP = B * ((H + 1) // 2) * ((W + 1) // 2)
    run, RP, nbx, L = ops.stemconv_wgrad_geometry(B, H, W, cin, cout)
    assert RP == 256 // (cout // 4) and 1 <= nbx <= 512
    assert L == run + _depth(RP) + -(-nbx // 64) + 6, (run, RP, nbx, L)
    assert run * nbx * RP >= NP > (run - 1) * nbx * RP, (run, RP, nbx, NP)


def test_geometry_bad_shapes():
    _lib, _, _ = _pkg()
    L = _lib.lib()
    out = (ctypes.c_int32 * 4)()
    for bad in ((0, 8, 1), (4, 12, 1), (4, 0, 1), (4, 520, 1), (4, 8, 0), (4, 8, 65)):
        assert L.obb_headconv_bwd_geometry(*bad, out) != 0, bad
    assert L.obb_headconv_bwd_geometry(4, 8, 1, None) != 0 and L.obb_headconv_bwd_geometry(4, 8, 1, out) == 0
    for bad in ((0, 4, 4, 3, 8), (1, 0, 4, 3, 8), (1, 4, 0, 3, 8), (1, 4, 4, 5, 8), (1, 4, 4, 2, 8), (1, 4, 4, 3, 12), (1, 4, 4, 3, 0), (1, 4, 4, 3, 72)):
        assert L.obb_stemconv_wgrad_geometry(*bad, out) != 0, bad
    assert L.obb_stemconv_wgrad_geometry(1, 4, 4, 3, 8, None) != 0 and L.obb_stemconv_wgrad_geometry(1, 4, 4, 3, 8, out) == 0


# ---------------------------------------------------------------------------------------------- the boundary
def test_new_ops_are_registered_and_refuse_cpu_tensors_and_bad_shapes():
    _, ops, TR = _pkg()
    for op in ("headconv_fwd", "headconv_bwd", "stemconv_fwd", "stemconv_wgrad"):
        assert hasattr(torch.ops.obbhip, op), f"torch.ops.obbhip.{op} is not registered"
    for cls in ("StemConvBN", "HeadOut", "DetectClassBranchStep", "DetectAngleBranch"):
        assert callable(getattr(TR, cls, None)), cls
    x, w, b = torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16), torch.zeros(3, 8), torch.zeros(3)
    dy = torch.zeros(1, 4, 4, 3)
    u8, ws, dz = torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(8, 3, 3, 3), torch.zeros(1, 2, 2, 8, dtype=torch.bfloat16)
    for call in (lambda: ops.headconv_fwd_bf16(x, w, b), lambda: ops.headconv_bwd_bf16(x, dy, w), lambda: ops.stemconv_fwd_u8(u8, ws),
                 lambda: ops.stemconv_wgrad_u8(u8, dz)):
        with pytest.raises(ValueError, match="no CPU path"):  # no quiet fall-back
            call()
    with pytest.raises(ValueError, match="3 or 4"):
        TR.StemConvBN(TR.ParamGroups(), torch.zeros(16, 5, 3, 3))
    with pytest.raises(ValueError, match="multiple of 8"):
        TR.StemConvBN(TR.ParamGroups(), torch.zeros(12, 3, 3, 3))
    with pytest.raises(ValueError, match="HeadOut"):
        TR.HeadOut(TR.ParamGroups(), torch.zeros(12, 64, 3, 3), torch.zeros(12))
    with pytest.raises(ValueError, match="HeadOut"):
        TR.HeadOut(TR.ParamGroups(), torch.zeros(65, 64, 1, 1), torch.zeros(65))
    with pytest.raises(ValueError, match="HeadOut"):
        TR.HeadOut(TR.ParamGroups(), torch.zeros(12, 60, 1, 1), torch.zeros(12))


# ---------------------------------------------------------------------------------------------- the measured tolerances
def _e(run, case):
    plain, rounded = run(case, False), run(case, True)
    return {n: NR.rel_dist(rounded[n], plain[n]) for n in plain}


def _in_band(e, measured):
    assert set(e) == set(measured), set(e) ^ set(measured)
    for n, v in e.items():
        assert measured[n] / 1.5 <= v <= measured[n] * 1.5, (n, v, measured[n])


@pytest.mark.parametrize("name,case,run,measured", [("stem", NR.stem_case, NR.run_stem, NR.E_STEM), ("head", NR.head_case, NR.run_head, NR.E_HEAD),
                                                    ("angle", NR.angle_case, NR.run_angle, NR.E_ANGLE), ("class", NR.class_case, NR.run_class, NR.E_CLASS)])
def test_rounded_against_plain(name, case, run, measured):
    e = _e(run, case())
    print(name + ": " + ", ".join(f'"{n}": {v:.2e}' for n, v in e.items()))
    _in_band(e, measured)


def test_plain_module_references_are_the_per_element_references():
    """The nn-module stacks (plain) agree with the per-element references on the same values: one definition of the layers, not two."""
    head, x, dy = NR.head_case()
    got = NR.run_head((head, x, dy), False)
    w, b = head.init[0].double().view(head.init[0].shape[0], -1), head.init[1].double()
    dx, dw, db = NR.head_bwd_ref(x.double(), dy.double(), w)
    for name, a, r in (("out", got["out"], _nchw(NR.head_fwd_ref(x.double(), w, b))), ("dx", got["dx"], _nchw(dx)), ("dW", got["dW"].view(dw.shape), dw),
                       ("db", got["db"], db)):
        assert float((a - r).abs().max()) <= 1e-12 * float(r.abs().max()), name
