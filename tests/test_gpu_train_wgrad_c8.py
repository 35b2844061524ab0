"""The weight gradient at channel counts that are multiples of 8 (csrc/convgrad.hip: k_conv_wgrad / obb_conv_wgrad_c8_bf16,
ops.conv_wgrad_c8_bf16) and `train.ConvBN` / `train.ClassBranchPair` on top of it, against fp64 references on the CPU computed from the same
bf16 values the device sees.

dW is an fp32 sum of K = B Ho Wo exact products (bf16 x bf16 is exact in fp32): in any summation order
    |got - ref| <= K u / (1 - K u) sum|x||dy|   per element,   u = 2^-24.
Every output goes into a buffer with 4 KiB guard bands of 0xff bytes (a NaN in fp32): afterwards every element is finite and both guards are
unchanged; every shape runs three times around a larger call that grows the slab slot, first and third result bit-identical."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import wgrad_c8_cases as WC
from bounds import Guarded, U, _check, _same_thrice

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.03  # Ultralytics' BatchNorm settings


def _mods():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    import oriented_object_detection_amd.train as TR
    return ops, _lib, TR


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _out_map(c):
    return ((c.H + 1) // 2, (c.W + 1) // 2) if c.s == 2 else (c.H, c.W)


def _refs(x, dy, c):
    """fp64 dW and sum |x||dy| of NCHW x, dy (the values the device sees)."""
    shape, p = (c.c2, c.c1, c.k, c.k), c.k // 2
    return (torch.nn.grad.conv2d_weight(x, shape, dy, stride=c.s, padding=p),
            torch.nn.grad.conv2d_weight(x.abs(), shape, dy.abs(), stride=c.s, padding=p))


def _run_guarded(ops, xd, dyd, c, what):
    dw = Guarded((c.c2, c.c1, c.k, c.k), torch.float32)
    ops.conv_wgrad_c8_bf16(xd, dyd, c.k, stride=c.s, out=dw.out)
    return dw.get(what)


@pytest.mark.parametrize("c", WC.GPU_CASES, ids=[WC.case_id(c) for c in WC.GPU_CASES])
def test_wgrad_c8(c):
    ops, _, _ = _mods()
    Ho, Wo = _out_map(c)
    g = torch.Generator().manual_seed(c.k * 1000003 + c.s * 100003 + c.c1 * 1009 + c.c2 * 101 + c.B * 31 + c.H * 7 + c.W)
    x = (torch.randn((c.B, c.c1, c.H, c.W), generator=g) * 0.7).bfloat16().double()
    dy = torch.randn((c.B, c.c2, Ho, Wo), generator=g).bfloat16().double()
    xd, dyd = _nhwc(x).bfloat16().cuda(), _nhwc(dy).bfloat16().cuda()
    ref, mag = _refs(x, dy, c)
    K = c.B * Ho * Wo
    run = lambda: _run_guarded(ops, xd, dyd, c, WC.case_id(c))
    _check("wgrad c8", run(), ref, K * U / (1 - K * U) * mag)
    xg = torch.randn((c.B + 2, c.H, c.W, c.c1), device="cuda").bfloat16()
    dyg = torch.randn((c.B + 2, Ho, Wo, 2 * c.c2), device="cuda").bfloat16()
    _same_thrice("wgrad c8", run, lambda: ops.conv_wgrad_c8_bf16(xg, dyg, c.k, stride=c.s))


@pytest.mark.parametrize("kind", ["onehot", "integers"])
@pytest.mark.parametrize("c", WC.EXACT_CASES, ids=[WC.case_id(c) for c in WC.EXACT_CASES])
def test_wgrad_c8_known_answer(c, kind):
    """Small-integer inputs: every product and every partial sum is an integer below 2^24, so the fp32 result equals the fp64 reference exactly,
    whatever the summation order.  onehot: x all ones, dy one at a single pixel and channel -- dW[co] is the indicator of the taps that land
    inside the map.  integers: x = ci + 1 + 3 (pixel index mod 5) (<= 28), dy = (co + 1)(1 + (y + 2 x + b) mod 3) (<= 24): a swapped tap, row
    or channel changes the sums (16 -> 8: |products| <= 672; 64 -> 64: x <= 76, dy <= 192, |products| <= 14592; K <= 234 terms)."""
    ops, _, _ = _mods()
    Ho, Wo = _out_map(c)
    if kind == "onehot":
        x = torch.ones((c.B, c.c1, c.H, c.W), dtype=torch.float64)
        dy = torch.zeros((c.B, c.c2, Ho, Wo), dtype=torch.float64)
        dy[1, 5, 0, Wo - 1] = 1.0  # top-right corner: the taps above and to the right fall into the padding
    else:
        pix = torch.arange(c.H * c.W).reshape(1, 1, c.H, c.W)
        x = (torch.arange(c.c1).reshape(1, -1, 1, 1) + 1 + 3 * (pix % 5)).expand(c.B, -1, -1, -1).double().contiguous()
        yy, xx, bb = torch.arange(Ho).reshape(1, 1, -1, 1), torch.arange(Wo).reshape(1, 1, 1, -1), torch.arange(c.B).reshape(-1, 1, 1, 1)
        dy = ((torch.arange(c.c2).reshape(1, -1, 1, 1) + 1) * (1 + (yy + 2 * xx + bb) % 3)).double().contiguous()
    assert torch.equal(x.bfloat16().double(), x) and torch.equal(dy.bfloat16().double(), dy)
    ref, mag = _refs(x, dy, c)
    assert float(mag.max()) < 2 ** 24
    got = _run_guarded(ops, _nhwc(x).bfloat16().cuda(), _nhwc(dy).bfloat16().cuda(), c, kind)
    if kind == "onehot":
        assert float(ref[5].sum()) == c.c1 * (1 if c.k == 1 else 4) and float(ref.sum()) == float(ref[5].sum())
    assert torch.equal(got.double().cpu(), ref), f"{kind}: {int((got.double().cpu() != ref).sum())} of {ref.numel()} elements differ"


@pytest.mark.parametrize("c", WC.ENTRY_EQUALITY_CASES, ids=[WC.case_id(c) for c in WC.ENTRY_EQUALITY_CASES])
def test_wgrad_entry_points_agree_at_multiples_of_64(c):
    """ops.conv_wgrad_bf16 and ops.conv_wgrad_c8_bf16 are two checks in front of one launcher: the same bits."""
    ops, _, _ = _mods()
    Ho, Wo = _out_map(c)
    g = torch.Generator().manual_seed(c.k * 1000003 + c.s * 100003 + c.c1 * 1009 + c.c2 * 101 + c.B * 31 + c.H * 7 + c.W)
    x = (torch.randn((c.B, c.H, c.W, c.c1), generator=g) * 0.7).bfloat16().cuda()
    dy = torch.randn((c.B, Ho, Wo, c.c2), generator=g).bfloat16().cuda()
    a, b = ops.conv_wgrad_bf16(x, dy, c.k, stride=c.s), ops.conv_wgrad_c8_bf16(x, dy, c.k, stride=c.s)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ"


@pytest.mark.parametrize("k,c1,c2", [(3, 64, 64), (1, 64, 128)])
def test_host_packed_dgrad_equals_the_device_packed_forward(k, c1, c2):
    """obb_conv_dgrad_bf16 (weights flipped, transposed and packed on the host) and ops.conv_fwd_bf16 on conv_pack_bf16(..., dgrad_form=True)
    share one packing and one launch: the same bits."""
    ops, _lib, _ = _mods()
    B, H, W = 2, 13, 9
    g = torch.Generator().manual_seed(k * 1009 + c1 * 101 + c2)
    w = torch.randn((c2, c1, k, k), generator=g) / (c1 * k * k) ** 0.5
    dy = torch.randn((B, H, W, c2), generator=g).bfloat16().cuda()
    host = ops.conv_dgrad_bf16(dy, w)
    dev = ops.conv_fwd_bf16(dy, ops.conv_pack_bf16(w.cuda(), H, W, dgrad_form=True), None, c1, k)
    torch.cuda.synchronize()
    assert host.shape == (B, H, W, c1) and bool(torch.isfinite(host.float()).all()) and float(host.float().abs().max()) > 0
    assert torch.equal(host, dev), f"{int((host != dev).sum())} of {host.numel()} elements differ"


REFUSALS = [
    # (what, B, H, W, cin, cout, ks, stride, message)
    ("cin 12", 1, 4, 4, 12, 16, 3, 1, "multiples of 8"),
    ("cout 4", 1, 4, 4, 16, 4, 3, 1, "multiples of 8"),
    ("cin 0", 1, 4, 4, 0, 16, 3, 1, "multiples of 8"),
    ("ks 5", 1, 4, 4, 16, 16, 5, 1, "are built"),
    ("stride 2 with ks 1", 1, 4, 4, 16, 16, 1, 2, "are built"),
    ("stride 3", 1, 4, 4, 16, 16, 3, 3, "are built"),
    ("B 0", 0, 4, 4, 16, 16, 3, 1, "bad arguments"),
    # one 400-pixel row at stride 2 with 64 channels per side: 3 x 401 + 200 pixels of 128 bytes = 175 KiB, more than a CU's LDS
    ("row too wide", 1, 2, 400, 64, 64, 3, 2, "does not fit"),
]


@pytest.mark.parametrize("what,B,H,W,cin,cout,ks,stride,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_wgrad_c8_refusals(what, B, H, W, cin, cout, ks, stride, msg):
    """OBB_ERR_INVALID with a message, and nothing written: the output and its guards stay 0xff."""
    ops, _lib, _ = _mods()
    x = torch.zeros(max(B, 1) * H * W * 64, dtype=torch.bfloat16, device="cuda")
    dy = torch.zeros(max(B, 1) * H * W * 64, dtype=torch.bfloat16, device="cuda")
    dw = Guarded((64, 64, 5, 5), torch.float32)
    with pytest.raises(_lib.ObbHipError, match=msg) as ei:
        ops._call("obb_conv_wgrad_c8_bf16", ops.ctx(x.device), ops._p(x), ops._p(dy), B, H, W, cin, cout, ks, stride, ops._p(dw.out), ops._stream())
    assert "libobbhip error -1:" in str(ei.value)  # OBB_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((dw.raw == 0xFF).all()), f"{what}: the refused call wrote into its output"


def test_wgrad_c8_null_buffers_and_wrapper_checks():
    ops, _lib, _ = _mods()
    x = torch.zeros(1, 4, 4, 16, dtype=torch.bfloat16, device="cuda")
    dy = torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16, device="cuda")
    dw = Guarded((8, 16, 3, 3), torch.float32)
    for args in ((None, dy, dw.out), (x, None, dw.out), (x, dy, None)):
        with pytest.raises(_lib.ObbHipError, match="NULL buffer"):
            ops._call("obb_conv_wgrad_c8_bf16", ops.ctx(x.device), ops._p(args[0]), ops._p(args[1]), 1, 4, 4, 16, 8, 3, 1, ops._p(args[2]), ops._stream())
    torch.cuda.synchronize()
    assert bool((dw.raw == 0xFF).all())
    with pytest.raises(ValueError, match="does not match"):
        ops.conv_wgrad_c8_bf16(x, dy, 3, stride=2)
    with pytest.raises(ValueError, match="wrong shape"):
        ops.conv_wgrad_c8_bf16(x, dy, 3, out=torch.zeros(8, 16, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="stride"):
        ops.conv_wgrad_c8_bf16(x, dy, 1, stride=2)
    # the 64-wide entry points refuse these layers as before, and write nothing
    with pytest.raises(_lib.ObbHipError, match="multiples of 64"):
        ops.conv_wgrad_bf16(x, dy, 3, out=dw.out)
    torch.cuda.synchronize()
    assert bool((dw.raw == 0xFF).all())


# ---------------------------------------------------------------------------------------------- train.ConvBN on narrow layers
def _q(t):
    """bf16 rounding point with a straight-through gradient (fp64 around it)."""
    return t + (t.to(torch.bfloat16).to(t.dtype) - t).detach()


def _nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _ref_block(c1, c2, k, s, g):
    ref = nn.Sequential(nn.Conv2d(c1, c2, k, s, k // 2, bias=False), nn.BatchNorm2d(c2, eps=EPS, momentum=MOM), nn.SiLU()).double().train()
    with torch.no_grad():
        ref[0].weight.copy_(torch.randn(c2, c1, k, k, generator=g) * (1.5 / (c1 * k * k) ** 0.5))
        ref[1].weight.copy_(torch.rand(c2, generator=g) + 0.5)
        ref[1].bias.copy_(torch.randn(c2, generator=g) * 0.2)
        ref[1].running_mean.copy_(torch.randn(c2, generator=g) * 0.1)
        ref[1].running_var.copy_(torch.rand(c2, generator=g) + 0.5)
    return ref


@pytest.mark.parametrize("k,s,c1,c2,B,H,W", WC.CONVBN_CASES)
@pytest.mark.parametrize("opt", ["SGD", "AdamW"])
def test_convbn_narrow_matches_torch_module(k, s, c1, c2, B, H, W, opt):
    """train.ConvBN at layers whose dW takes the c8 route, against Conv2d(bias=False) -> BatchNorm2d(eps 1e-3, momentum 0.03) -> SiLU in .train()
    in fp64 at the device's bf16 rounding points (weights, z, a), by test_gpu_train_bn.py's criterion for ConvBN: max |d| / max |ref| of the
    output, dx, dW, dgamma, dbeta and the running statistics, then one optimiser step of the three groups against torch.optim on the same
    gradients."""
    ops, _, TR = _mods()
    assert TR.wgrad_route(c1, c2) == "c8"
    g = torch.Generator().manual_seed(B * 100 + H + c1 + k + s)
    ref = _ref_block(c1, c2, k, s, g)
    x = torch.randn(B, H, W, c1, generator=g).to(torch.bfloat16)
    Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
    da = (torch.randn(B, Ho, Wo, c2, generator=g) * 0.1).to(torch.bfloat16)

    lr, wd = (0.01 if opt == "SGD" else 0.001), 5e-4
    grp = TR.ParamGroups(opt, lr=lr, momentum=0.9, weight_decay=wd)
    blk = TR.ConvBN(grp, ref[0].weight.detach().float().cuda(), ref[1].weight.detach().float().cuda(), ref[1].bias.detach().float().cuda(), s=s,
                    running_mean=ref[1].running_mean.float().cuda(), running_var=ref[1].running_var.float().cuda())
    grp.build()
    a = blk.forward(x.cuda())
    dx = blk.backward(da.cuda())
    torch.cuda.synchronize()

    xr = _nchw(x).requires_grad_(True)
    z = _q(F.conv2d(xr, _q(ref[0].weight), stride=s, padding=k // 2))
    a_ref = _q(ref[2](ref[1](z)))
    a_ref.backward(_nchw(da))
    rel = lambda d, r: float((d.double() - r).abs().max()) / float(r.abs().max())
    e = {"a": rel(_nchw(a), a_ref.detach()), "dx": rel(_nchw(dx), xr.grad), "dW": rel(blk.dw.cpu(), ref[0].weight.grad),
         "dgamma": rel(blk.dgamma.cpu(), ref[1].weight.grad), "dbeta": rel(blk.dbeta.cpu(), ref[1].bias.grad),
         "rmean": rel(blk.running_mean.cpu(), ref[1].running_mean), "rvar": rel(blk.running_var.cpu(), ref[1].running_var)}
    print(f"{B}x{H}x{W} {c1}->{c2} k{k} s{s}: " + ", ".join(f"{n} {v:.2e}" for n, v in e.items()))
    assert e["a"] <= 1.2e-2 and e["dx"] <= 1.2e-2, e
    assert e["dW"] <= 8e-3, e
    assert e["dgamma"] <= 1e-3 and e["dbeta"] <= 1e-3, e
    assert e["rmean"] <= 1e-5 and e["rvar"] <= 1e-5, e

    params = [nn.Parameter(p.detach().float().clone()) for p in (ref[0].weight, ref[1].weight, ref[1].bias)]
    groups = [{"params": [params[0]], "weight_decay": wd}, {"params": [params[1]], "weight_decay": 0.0}, {"params": [params[2]], "weight_decay": 0.0}]
    topt = (torch.optim.SGD(groups, lr=lr, momentum=0.9, nesterov=True, foreach=False) if opt == "SGD"
            else torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), foreach=False))
    for p, gr in zip(params, (blk.dw, blk.dgamma, blk.dbeta)):
        p.grad = gr.cpu().clone()
    topt.step()
    grp.step()
    for p, d in zip(params, (blk.w, blk.gamma, blk.beta)):
        assert float((d.cpu() - p.detach()).abs().max()) <= 2e-6 * max(1.0, float(p.detach().abs().max()))


def test_convbn_64_multiples_keep_the_c64_route():
    """A 64 -> 64 ConvBN writes the dW that a direct ops.conv_wgrad_bf16 call on its (x, dz) gives, bit for bit."""
    ops, _, TR = _mods()
    assert TR.wgrad_route(64, 64) == "c64"
    g = torch.Generator().manual_seed(64)
    B, H, W = 2, 13, 9
    grp = TR.ParamGroups("SGD")
    blk = TR.ConvBN(grp, (torch.randn(64, 64, 3, 3, generator=g) * 0.06).cuda(), (torch.rand(64, generator=g) + 0.5).cuda(),
                    (torch.randn(64, generator=g) * 0.2).cuda())
    grp.build()
    x = torch.randn(B, H, W, 64, generator=g).to(torch.bfloat16).cuda()
    da = (torch.randn(B, H, W, 64, generator=g) * 0.1).to(torch.bfloat16).cuda()
    blk.forward(x)
    blk.backward(da)
    _, z, mean, invstd = blk.saved
    dz, _, _ = ops.bn_silu_bwd_bf16(z, da, blk.gamma, blk.beta, mean, invstd)
    direct = ops.conv_wgrad_bf16(x, dz, 3)
    torch.cuda.synchronize()
    assert torch.equal(blk.dw, direct)
    assert bool(torch.isfinite(blk.dw).all()) and float(blk.dw.abs().max()) > 0


def test_class_branch_pair_trains_with_a_narrow_pointwise_conv():
    """ClassBranchPair(DWConv 3x3 on 64 channels, Conv 1x1 64 -> 32): the pointwise dW (c8 route) against the fp64 bound from the block's own
    saved (x, dz); every gradient finite and non-zero, dx of the input's shape."""
    ops, _, TR = _mods()
    g = torch.Generator().manual_seed(23)
    B, H, W, c1, c2 = 2, 13, 9, 64, 32
    grp = TR.ParamGroups("SGD")
    pair = TR.ClassBranchPair(grp, ((torch.randn(c1, 1, 3, 3, generator=g) * 0.3).cuda(),), ((torch.randn(c2, c1, 1, 1, generator=g) * 0.15).cuda(),))
    grp.build()
    x = torch.randn(B, H, W, c1, generator=g).to(torch.bfloat16).cuda()
    da = (torch.randn(B, H, W, c2, generator=g) * 0.1).to(torch.bfloat16).cuda()
    assert pair.forward(x).shape == (B, H, W, c2)
    dx = pair.backward(da)
    torch.cuda.synchronize()
    assert dx.shape == x.shape
    for t in (pair.dw.dw, pair.dw.dgamma, pair.dw.dbeta, pair.pw.dw, pair.pw.dgamma, pair.pw.dbeta, dx):
        assert bool(torch.isfinite(t.float()).all()) and float(t.float().abs().max()) > 0
    xin, z, mean, invstd = pair.pw.saved
    dz, _, _ = ops.bn_silu_bwd_bf16(z, da, pair.pw.gamma, pair.pw.beta, mean, invstd)
    c = WC.Case("pair", 1, 1, c1, c2, B, H, W)
    ref, mag = _refs(_nchw(xin), _nchw(dz), c)
    K = B * H * W
    _check("ClassBranchPair pw dW", pair.pw.dw, ref, K * U / (1 - K * U) * mag)
