"""CPU checks of the depthwise Conv-block slice (csrc/dwgrad.hip, the `act` flag of csrc/bntrain.hip): the fp64 references of tests/dw_ref.py
against torch.autograd, the boundary (header, ctypes signatures, ops wrappers, train blocks), the launcher's own work split through the host-only
obb_dwconv3_bwd_geometry, and the rounded-against-plain measurement that sets the tolerances of the assembled GPU tests.  No GPU."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dw_ref as DR
from conftest import ROOT

MAPS = [(13, 9), (5, 7), (4, 4), (1, 1), (2, 1), (1, 2)]
NEW = ["obb_dwconv3_fwd_bf16", "obb_dwconv3_bwd_bf16", "obb_dwconv3_bwd_geometry", "obb_bn_fwd_bf16", "obb_bn_bwd_bf16"]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("H,W", MAPS)
def test_dw_references_equal_autograd(H, W):
    """dw_fwd_ref / dw_bwd_ref against autograd through F.conv2d(groups=C, padding=1) in fp64, to 1e-12 of the largest entry."""
    B, C = 2, 5
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    dz = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(C, 1, 3, 3, generator=g, dtype=torch.float64)
    xr, wr = _nchw(x).clone().requires_grad_(True), w.clone().requires_grad_(True)
    z = F.conv2d(xr, wr, padding=1, groups=C)
    z.backward(_nchw(dz))
    dx, dw = DR.dw_bwd_ref(x, dz, w)
    for name, got, ref in (("z", _nchw(DR.dw_fwd_ref(x, w)), z.detach()), ("dx", _nchw(dx), xr.grad), ("dw", dw, wr.grad)):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name


@pytest.mark.parametrize("act", [False, True])
def test_bn_ref_equals_batch_norm(act):
    g = torch.Generator().manual_seed(5 + act)
    z = torch.randn(2, 7, 5, 6, generator=g, dtype=torch.float64) * 1.5 + 0.3
    gamma, beta = torch.rand(6, generator=g, dtype=torch.float64) + 0.5, torch.randn(6, generator=g, dtype=torch.float64)
    y = F.batch_norm(z.reshape(-1, 6), None, None, gamma, beta, training=True, eps=DR.EPS)
    ref = (F.silu(y) if act else y).reshape(z.shape)
    assert float((DR.bn_ref(z, gamma, beta, DR.EPS, act) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_dw_boundary_is_declared_bound_and_wrapped():
    """The five entry points are in the header and in _lib.SIGNATURES (with the header's argument counts), ops has the wrappers and the
    registered ops, train has the blocks, and a CPU tensor raises instead of taking another path."""
    hdr = open(os.path.join(ROOT, "include", "obbhip.h")).read()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    import oriented_object_detection_amd.train as TR
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/obbhip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert len(_lib.SIGNATURES[name]) == len(m.group(1).split(",")), name
    for fn in ("dwconv3_fwd_bf16", "dwconv3_bwd_bf16", "bn_fwd_bf16", "bn_bwd_bf16", "dwconv3_bwd_geometry"):
        assert callable(getattr(ops, fn, None)), f"ops.{fn} is missing"
    for op in ("dwconv3_fwd", "dwconv3_bwd", "bn_fwd", "bn_bwd"):
        assert hasattr(torch.ops.obbhip, op), f"torch.ops.obbhip.{op} is not registered"
    assert callable(getattr(TR, "DWConvBN", None)) and callable(getattr(TR, "ClassBranchPair", None))
    with pytest.raises(ValueError, match=r"\[C,1,3,3\]"):
        TR.DWConvBN(TR.ParamGroups(), torch.zeros(8, 8, 3, 3))
    x = torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16)
    w, v = torch.zeros(8, 1, 3, 3), torch.ones(8)
    with pytest.raises(ValueError, match="no CPU path"):  # no quiet fall-back
        ops.dwconv3_fwd_bf16(x, w)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.dwconv3_bwd_bf16(x, x, w)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.bn_fwd_bf16(x, v, v, v, v, act=False)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.bn_bwd_bf16(x, x, v, v, v, v, act=False)


@pytest.mark.parametrize("B,H,W,C", DR.DW_SHAPES)
def test_bwd_geometry_of_every_gpu_shape(B, H, W, C):
    """The launcher's split at every shape of the GPU test: L <= 96, at least one slab, stripes that cover H exactly, the same answer twice."""
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    rows, run, slabs, L = ops.dwconv3_bwd_geometry(B, H, W, C)
    assert (rows, run, slabs, L) == ops.dwconv3_bwd_geometry(B, H, W, C)
    assert 1 <= L <= 96 and slabs >= 1 and rows >= 1 and run >= rows and run % rows == 0, (rows, run, slabs, L)
    stripes = [(i0, min(i0 + rows, H)) for i0 in range(0, H, rows)]
    assert stripes[0][0] == 0 and stripes[-1][1] == H and all(a[1] == b[0] for a, b in zip(stripes, stripes[1:])) and all(b > a for a, b in stripes)
    assert sum(b - a for a, b in stripes) == H


def test_bwd_geometry_branches_and_bad_shapes():
    """The shapes of dw_ref.BRANCHES sit where their comments say, and a bad shape is an error code, not a split."""
    import ctypes
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    assert ops.dwconv3_bwd_geometry(2, 16, 16, 64)[0] == 2 and ops.dwconv3_bwd_geometry(1, 17, 3, 8)[0] == 4
    assert ops.dwconv3_bwd_geometry(1, 1, 1, 8)[2] == 1 and ops.dwconv3_bwd_geometry(2, 13, 13, 64)[2] > 1
    rows, run, slabs, _ = ops.dwconv3_bwd_geometry(2, 16, 260, 256)
    assert run == 2 * rows and slabs == 512
    assert all(ops.dwconv3_bwd_geometry(*s)[1] == ops.dwconv3_bwd_geometry(*s)[0] for s in DR.CATALOGUE + DR.EDGES)
    out = (ctypes.c_int32 * 4)()
    for bad in ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 12), (1, 4, 4, 0)):
        assert _lib.lib().obb_dwconv3_bwd_geometry(*bad, out) != 0, bad
    assert _lib.lib().obb_dwconv3_bwd_geometry(1, 4, 4, 8, None) != 0


# The tolerances of the assembled GPU tests.  e = max |rounded - plain| / max |plain| per tensor, where `plain` is the nn-module reference in
# fp64 with no rounding and `rounded` the same evaluation with a bf16 rounding at each of the device's rounding points (x, the weights, z, a,
# da, dz, dx).  test_gpu_train_dw.py recomputes e from the same functions and requires the device within 2 e of plain.  The bands below are
# [1 / 1.5, 1.5] x the figures measured here (fp64 on the CPU; a different summation order moves them in the 12th digit): a change of the
# emulation -- a rounding point dropped or added -- moves a figure by far more and is seen here, not as a looser GPU test.
E_DWBN = {
    (2, 26, 26, 128, True): {"out": 5.00e-3, "dx": 3.75e-3, "dW": 2.67e-3, "dgamma": 2.34e-3, "dbeta": 1.35e-3, "rmean": 3.76e-5, "rvar": 2.86e-4},
    # no activation: dbeta is the plain sum of da, which no rounding point touches -- e = 0, and the device has to be exact (dw_ref._grad_in)
    (2, 13, 13, 128, False): {"out": 4.27e-3, "dx": 4.82e-3, "dW": 2.01e-3, "dgamma": 2.50e-3, "dbeta": 0.0, "rmean": 7.12e-5, "rvar": 2.56e-4},
}
E_PAIR = {"out": 5.73e-3, "dx": 5.18e-3, "dw.dW": 5.44e-3, "dw.dgamma": 4.46e-3, "dw.dbeta": 4.99e-3, "dw.rmean": 3.18e-5, "dw.rvar": 3.08e-4,
          "pw.dW": 4.92e-3, "pw.dgamma": 3.42e-3, "pw.dbeta": 1.48e-3, "pw.rmean": 1.39e-4, "pw.rvar": 2.56e-5}


def _e(run, case):
    plain, rounded = run(case, False), run(case, True)
    return {n: DR.rel_dist(rounded[n], plain[n]) for n in plain}


def _in_band(e, measured):
    assert set(e) == set(measured), set(e) ^ set(measured)
    for n, v in e.items():
        assert measured[n] / 1.5 <= v <= measured[n] * 1.5, (n, v, measured[n])


@pytest.mark.parametrize("B,H,W,C,act", list(E_DWBN))
def test_rounded_against_plain_dwconvbn(B, H, W, C, act):
    e = _e(DR.run_dwbn, DR.dwbn_case(B, H, W, C, act))
    print(", ".join(f"{n} {v:.3e}" for n, v in e.items()))
    _in_band(e, E_DWBN[(B, H, W, C, act)])


def test_rounded_against_plain_class_branch_pair():
    e = _e(DR.run_pair, DR.pair_case(2, 26, 26, 128, 64))
    print(", ".join(f"{n} {v:.3e}" for n, v in e.items()))
    _in_band(e, E_PAIR)
