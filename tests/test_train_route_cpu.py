"""CPU checks of the gradient-routing slice (csrc/routegrad.hip): the fp64 references of tests/route_ref.py against torch.autograd on inputs
full of ties, and the boundary (header, ctypes signatures, ops wrappers, train blocks).  No GPU."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import route_ref as RR
from conftest import ROOT

SHAPES = [(13, 13), (4, 4), (7, 5), (1, 1), (2, 1)]
NEW = ["obb_sppf_pools_fwd_bf16", "obb_sppf_pools_bwd_bf16", "obb_upcat_fwd_bf16", "obb_upcat_bwd_bf16"]


def _inputs(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    quant = torch.round(torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * 4) / 4  # multiples of 0.25: many ties in every window
    return {"quantised": quant, "constant": torch.full((B, H, W, C), 0.75, dtype=torch.float64), "negative": -quant.abs() - 0.25}


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("H,W", SHAPES)
def test_pool_references_equal_autograd_on_ties(H, W):
    """pools_ref / pools_bwd_ref (first maximum in row-major scan) are EXACTLY what autograd gives through
    cat([x, p(x), p(p(x)), p(p(p(x)))]) in fp64: forward bit-equal, backward bit-equal (gradients are multiples of 2^-6: every sum is exact)."""
    B, C = 2, 3
    g = torch.Generator().manual_seed(H * 10 + W)
    dcat = torch.round(torch.randn(B, H, W, 4 * C, generator=g, dtype=torch.float64) * 64) / 64
    for name, x in _inputs(B, H, W, C, H * 31 + W).items():
        xr = _nchw(x).clone().requires_grad_(True)
        ys = [xr]
        for _ in range(3):
            ys.append(F.max_pool2d(ys[-1], 5, 1, 2))
        cat = torch.cat(ys, dim=1)
        cat.backward(_nchw(dcat))
        ref_cat = RR.pools_ref(x)
        assert torch.equal(_nchw(ref_cat), cat.detach()), name
        assert torch.equal(_nchw(RR.pools_bwd_ref(ref_cat, dcat)), xr.grad), name
        if name == "negative":
            assert float(ref_cat.max()) < 0  # a zero padding would have won


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("up", [1, 2])
def test_upcat_references_equal_autograd(H, W, up):
    """upcat_ref / upcat_bwd_ref against autograd through cat(interpolate(a, nearest), b) in fp64, plain and with prior buffers added, on the
    same three kinds of input (quantised gradients too: every sum is exact whatever its order)."""
    B, Ca, Cb = 2, 3, 5
    g = torch.Generator().manual_seed(H * 10 + W + up)
    qrand = lambda *s: torch.round(torch.randn(*s, generator=g, dtype=torch.float64) * 4) / 4
    dout = qrand(B, H * up, W * up, Ca + Cb)
    da0, db0 = qrand(B, H, W, Ca), qrand(B, H * up, W * up, Cb)
    for (name, a0), b0 in zip(_inputs(B, H, W, Ca, H * 31 + W + up).items(), _inputs(B, H * up, W * up, Cb, H * 17 + W + up).values()):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        au = _nchw(a) if up == 1 else F.interpolate(_nchw(a), scale_factor=up, mode="nearest")
        out = torch.cat([au, _nchw(b)], dim=1)
        out.backward(_nchw(dout))
        assert torch.equal(_nchw(RR.upcat_ref(a0, b0, up)), out.detach()), name
        da, db = RR.upcat_bwd_ref(dout, Ca, up)
        assert float((da - a.grad).abs().max()) <= 1e-15 and float((db - b.grad).abs().max()) <= 1e-15, name
        da2, db2 = RR.upcat_bwd_ref(dout, Ca, up, da0, db0)
        assert float((da2 - (a.grad + da0)).abs().max()) <= 1e-15 and float((db2 - (b.grad + db0)).abs().max()) <= 1e-15, name


def test_bf16_gradients_explain_cv1_dbeta():
    """Why test_gpu_train_route.py::test_sppf_block_matches_torch_modules measures cv1 dbeta at 1.54e-2 and dgamma at 1.09e-2 of max at
    2x13x13x256 although the kernels are within a rounding of fp64: the device stores every gradient tensor in bf16 (for cv1's dgamma / dbeta
    the ones that count are cv2's dz, dcat and the pools' dx), autograd rounds no gradient.  The SAME nn reference on the SAME seeded case, once as it is and once with a bf16 rounding of these gradients, differs
    from itself by the measured figures (cv1 dbeta 1.54e-2, dgamma 1.09e-2, dx 6.9e-3, cv1 dW 5.9e-3, cv2 dW 4.8e-3), and cv2's dgamma / dbeta,
    which lie above every one of these roundings, do not move at all.  The windows are wide because the CPU's fp32 convolution may order its
    sums differently from machine to machine; the figures only have to be of that size."""
    def run(grad_bf16):
        cv1, cv2, x, da = RR.sppf_case(2, 13, 13, 256, 256)
        xr = _nchw(x.float()).requires_grad_(True)
        _, out = RR.ref_sppf(cv1, cv2, xr, None, grad_bf16)
        out.backward(_nchw(da.float()))
        return {"dx": xr.grad, "cv1.dW": cv1.w.grad, "cv1.dgamma": cv1.bn.weight.grad, "cv1.dbeta": cv1.bn.bias.grad, "cv2.dW": cv2.w.grad,
                "cv2.dgamma": cv2.bn.weight.grad, "cv2.dbeta": cv2.bn.bias.grad}
    plain, rounded = run(False), run(True)
    e = {n: float((plain[n] - rounded[n]).abs().max() / plain[n].abs().max()) for n in plain}
    print(", ".join(f"{n} {v:.3e}" for n, v in e.items()))
    assert 1.2e-2 <= e["cv1.dbeta"] <= 1.9e-2, e
    assert 0.8e-2 <= e["cv1.dgamma"] <= 1.4e-2, e
    assert 5e-3 <= e["dx"] <= 9e-3 and 4e-3 <= e["cv1.dW"] <= 8e-3 and 3.5e-3 <= e["cv2.dW"] <= 6.5e-3, e
    assert e["cv2.dgamma"] == 0 and e["cv2.dbeta"] == 0, e


def test_route_boundary_is_declared_bound_and_wrapped():
    """The four entry points are in the header and in _lib.SIGNATURES (with the header's argument counts), ops has the wrappers and the registered
    ops, train has the blocks."""
    hdr = open(os.path.join(ROOT, "include", "obbhip.h")).read()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    import oriented_object_detection_amd.train as TR
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/obbhip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert len(_lib.SIGNATURES[name]) == len(m.group(1).split(",")), name
    for fn in ("sppf_pools_fwd_bf16", "sppf_pools_bwd_bf16", "upcat_fwd_bf16", "upcat_bwd_bf16"):
        assert callable(getattr(ops, fn, None)), f"ops.{fn} is missing"
    for op in ("sppf_pools_fwd", "sppf_pools_bwd", "upcat_fwd", "upcat_bwd"):
        assert hasattr(torch.ops.obbhip, op), f"torch.ops.obbhip.{op} is not registered"
    assert callable(getattr(TR, "SPPF", None)) and callable(getattr(TR, "UpCat", None))
    with pytest.raises(ValueError, match="up = 3"):
        TR.UpCat(3)
    x = torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="no CPU path"):  # no quiet fall-back
        ops.sppf_pools_fwd_bf16(x)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.upcat_fwd_bf16(x, x, 1)
