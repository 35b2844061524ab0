"""The training kernels at every YOLO11 n / s layer shape (train_shapes.py) and at off-catalogue edge shapes, against fp64 references on the
CPU computed from the same bf16 values the device sees.

Bounds are per element, never relative to a tensor's maximum.  u = 2^-24 (fp32 unit roundoff), u_bf = 2^-8 (bf16, round to nearest even).
  bf16 output of an fp32 sum of K exact products (bf16 x bf16 is exact in fp32): any summation order of K terms is within
    gamma_K sum|a||b|, gamma_K = K u / (1 - K u); rounding the result v = ref + e to bf16 adds u_bf |v| <= u_bf |ref| + u_bf |e|, so
    |got - ref| <= u_bf |ref| + c K u sum|a||b|, c = (1 + u_bf) / (1 - K u)  (<= 1.005 for every K here).
  fp32 output of a sum of K exact products (dW): |got - ref| <= K u / (1 - K u) sum|a||b|.
  fp32 reductions over pixels in fixed-order blocks (BN statistics / dgamma / dbeta, bias gradient): <= R sum of magnitudes, R = 1e-6
    (the blocked partial sums keep every running sum short; a serial fp32 walk over the pixels does not -- see test_bias_grad_large_offset).
Every output goes into a buffer with 4 KiB guard bands on both sides, all bytes 0xff (a NaN in bf16 and fp32): afterwards every output
element is finite and both guards are unchanged, bit for bit.  Each reduction runs three times: at the test's shape, at a larger shape that
grows its workspace slot, and at the test's shape again; the first and third results are identical."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import train_shapes as TS
from bounds import Guarded, _check, _same_thrice

pytestmark = pytest.mark.gpu

U, UBF = 2.0 ** -24, 2.0 ** -8
R = 1e-6
EPS, MOM = 1e-3, 0.03  # Ultralytics' BatchNorm settings
BF16_MAX = float(torch.finfo(torch.bfloat16).max)


def _ops():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    return ops, _lib


def _bf16_bound(ref, S, K):
    return UBF * ref.abs() + (1 + UBF) / (1 - K * U) * K * U * S


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _bf(t):
    return t.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- convolutions
CONV_CASES = TS.trained_convs() + TS.EDGE_CONVS


@pytest.mark.parametrize("e", CONV_CASES, ids=[e.id for e in CONV_CASES])
def test_conv_train_kernels(e):
    """Forward (+ bias), the input gradient in each form the layer can use, and wgrad (or its documented refusal) at one layer shape."""
    ops, _lib = _ops()
    k, s, c1, c2, B, H, W = e.k, e.s, e.c1, e.c2, e.B, e.H, e.W
    p = k // 2
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if s == 2 else (H, W)
    g = torch.Generator().manual_seed(zlib.crc32(e.id.encode()))
    x = _bf(torch.randn((B, c1, H, W), generator=g) * 0.7).double()
    w = _bf(torch.randn((c2, c1, k, k), generator=g) / math.sqrt(c1 * k * k)).double()
    bias = (torch.randn(c2, generator=g) * 0.1).float().double()
    dy = _bf(torch.randn((B, c2, Ho, Wo), generator=g)).double()
    print(f"{e.id}: k{k} s{s} {c1} -> {c2}, {B} x {H} x {W}")
    c = ops.ctx(torch.device("cuda"))
    st = ops._stream()
    xd, dyd = _nhwc(x).bfloat16().cuda(), _nhwc(dy).bfloat16().cuda()
    wd = w.float().cuda()

    # forward: K = c1 k^2 products + the bias
    y_ref = F.conv2d(x, w, bias, stride=s, padding=p)
    y_mag = F.conv2d(x.abs(), w.abs(), bias.abs(), stride=s, padding=p)
    pk = ops.conv_pack_bf16(wd, H, W, stride=s)
    y = Guarded((B, Ho, Wo, c2), torch.bfloat16)
    bd = bias.float().cuda()
    if s == 2:
        ops._call("obb_conv_fwd_s2_bf16", c, ops._p(xd), ops._p(pk), ops._p(bd), B, H, W, c1, c2, ops._p(y.out), st)
    else:
        ops._call("obb_conv_fwd_bf16", c, ops._p(xd), ops._p(pk), ops._p(bd), B, H, W, c1, c2, k, ops._p(y.out), st)
    _check("forward", _nchw(y.get("forward")), y_ref, _bf16_bound(y_ref, y_mag, c1 * k * k + 1))

    # input gradient: K = c2 k^2 products (the stride-2 form also sums the inserted zeros, which add exactly)
    dx_ref = torch.nn.grad.conv2d_input((B, c1, H, W), w, dy, stride=s, padding=p)
    dx_mag = torch.nn.grad.conv2d_input((B, c1, H, W), w.abs(), dy.abs(), stride=s, padding=p)
    dx_bound = _bf16_bound(dx_ref, dx_mag, c2 * k * k)
    pkd = ops.conv_pack_bf16(wd, H, W, dgrad_form=True)
    if s == 1:
        wh = w.float().contiguous()
        dx = Guarded((B, H, W, c1), torch.bfloat16)
        ops._call("obb_conv_dgrad_bf16", c, ops._p(dyd), wh.numpy().ctypes.data_as(_lib.c_fp), B, H, W, c1, c2, k, ops._p(dx.out), st)
        _check("dgrad, host-packed", _nchw(dx.get("dgrad host")), dx_ref, dx_bound)
        dx = Guarded((B, H, W, c1), torch.bfloat16)
        ops._call("obb_conv_fwd_bf16", c, ops._p(dyd), ops._p(pkd), None, B, H, W, c2, c1, k, ops._p(dx.out), st)
        _check("dgrad, device-packed forward (ConvBN)", _nchw(dx.get("dgrad device")), dx_ref, dx_bound)
    else:
        dx = Guarded((B, H, W, c1), torch.bfloat16)
        ops._call("obb_conv_dgrad_s2_bf16", c, ops._p(dyd), ops._p(pkd), B, H, W, c1, c2, ops._p(dx.out), st)
        _check("dgrad, stride 2", _nchw(dx.get("dgrad s2")), dx_ref, dx_bound)

    # weight gradient: a sum of K = B Ho Wo exact products per element, fp32 out
    dw = Guarded((c2, c1, k, k), torch.float32)
    if TS.conv_class(k, s, 1, c1, c2) != TS.WGRAD:
        with pytest.raises(_lib.ObbHipError, match="multiples of 64"):
            ops.conv_wgrad_bf16(xd, dyd, k, stride=s, out=dw.out)
        torch.cuda.synchronize()
        assert bool((dw.raw == 0xFF).all()), "refused wgrad wrote into its output"
        return
    K = B * Ho * Wo
    dw_ref = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=s, padding=p)
    dw_mag = torch.nn.grad.conv2d_weight(x.abs(), w.shape, dy.abs(), stride=s, padding=p)
    run = lambda: (ops.conv_wgrad_bf16(xd, dyd, k, stride=s, out=dw.out), dw.get("wgrad"))[1]
    _check("wgrad", run(), dw_ref, K * U / (1 - K * U) * dw_mag)
    xg = torch.randn((B + 2, H, W, c1), device="cuda").bfloat16()
    dyg = torch.randn((B + 2, Ho, Wo, 2 * c2), device="cuda").bfloat16()
    _same_thrice("wgrad", run, lambda: ops.conv_wgrad_bf16(xg, dyg, k, stride=s))


def _nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def test_packed_blob_for_another_map_is_refused():
    """plan_conv packs 3x3 64 -> 32 at 52 x 52 single-stage (WRES, CK = 64) and at 48 x 48 in 16-channel stages: a blob packed for one map size
    must not run at the other.  The dgrad form of a 32 -> 64 conv is the same logical 64 -> 32 conv.  (Stride-2 forward blobs do not depend on
    the map: plan_conv keeps CK = 16 there.)"""
    ops, _ = _ops()
    w = torch.randn(32, 64, 3, 3, device="cuda") * 0.05
    wt = torch.randn(64, 32, 3, 3, device="cuda") * 0.05
    x = torch.randn(1, 48, 48, 64, device="cuda").bfloat16()
    with pytest.raises(ValueError, match="packed"):
        ops.conv_fwd_bf16(x, ops.conv_pack_bf16(w, 52, 52), None, 32, 3)
    with pytest.raises(ValueError, match="packed"):  # the dgrad form through the forward, as ConvBN runs it
        ops.conv_fwd_bf16(x, ops.conv_pack_bf16(wt, 52, 52, dgrad_form=True), None, 32, 3)
    with pytest.raises(ValueError, match="packed"):
        ops.conv_dgrad_s2_bf16(torch.randn(1, 24, 24, 64, device="cuda").bfloat16(), ops.conv_pack_bf16(wt, 52, 52, dgrad_form=True), 32, 48, 48)
    # the matching blobs run
    assert ops.conv_fwd_bf16(x, ops.conv_pack_bf16(w, 48, 48), None, 32, 3).shape == (1, 48, 48, 32)
    assert ops.conv_fwd_bf16(x, ops.conv_pack_bf16(wt, 48, 48, dgrad_form=True), None, 32, 3).shape == (1, 48, 48, 32)


# ---------------------------------------------------------------------------------------------- BatchNorm(train) + SiLU
BN_CASES = [(e, None) for e in TS.trained_bns() + TS.EDGE_BNS] + [(e, "offset") for e in TS.EDGE_BNS if e.C in (8, 392)]


def _bn_inputs(e, mode, seed):
    g = torch.Generator().manual_seed(seed)
    C, npix = e.C, e.B * e.H * e.W
    if mode == "offset":  # |mean| >> std: a one-pass E[z^2] - E[z]^2 would cancel
        mu, sd = torch.full((C,), 8.0), torch.full((C,), 0.05)
    else:
        mu, sd = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) * 1.5 + 0.25
    z = torch.randn(npix, C, generator=g) * sd + mu
    z[:, 0] = 0.375  # a zero-variance channel: invstd = 1 / sqrt(eps), no NaN
    z = _bf(z).double()
    gamma = (torch.rand(C, generator=g) * 1.5 + 0.25).double()
    beta = (torch.randn(C, generator=g) * 0.3).double()
    rm, rv = (torch.randn(C, generator=g) * 0.1).double(), (torch.rand(C, generator=g) + 0.5).double()
    da = _bf(torch.randn(npix, C, generator=g) * 0.1).double()
    return z, gamma, beta, rm, rv, da


def _bn_fwd(ops, zd, gd, bd, rm, rv, C, npix):
    a, mean, inv = Guarded((npix, C), torch.bfloat16), Guarded((C,), torch.float32), Guarded((C,), torch.float32)
    rmg, rvg = Guarded((C,), torch.float32, rm), Guarded((C,), torch.float32, rv)
    ops._call("obb_bn_silu_fwd_bf16", ops.ctx(zd.device), ops._p(zd), npix, C, ops._p(gd), ops._p(bd), EPS, MOM, ops._p(rmg.out), ops._p(rvg.out),
              ops._p(mean.out), ops._p(inv.out), ops._p(a.out), ops._stream())
    return [t.get(n) for t, n in ((a, "a"), (mean, "mean"), (inv, "invstd"), (rmg, "running_mean"), (rvg, "running_var"))]


def _bn_bwd(ops, zd, dad, gd, bd, mean, inv, C, npix):
    dz, dg, db = Guarded((npix, C), torch.bfloat16), Guarded((C,), torch.float32), Guarded((C,), torch.float32)
    ops._call("obb_bn_silu_bwd_bf16", ops.ctx(zd.device), ops._p(zd), ops._p(dad), npix, C, ops._p(gd), ops._p(bd), ops._p(mean), ops._p(inv),
              ops._p(dg.out), ops._p(db.out), ops._p(dz.out), ops._stream())
    return [t.get(n) for t, n in ((dz, "dz"), (dg, "dgamma"), (db, "dbeta"))]


@pytest.mark.parametrize("e,mode", BN_CASES, ids=[e.id + (" offset" if m else "") for e, m in BN_CASES])
def test_bn_silu_train(e, mode):
    ops, _ = _ops()
    C, npix = e.C, e.B * e.H * e.W
    N = float(npix)
    print(f"{e.id} {mode or ''}: C {C}, npix {npix}")
    z, gamma, beta, rm, rv, da = _bn_inputs(e, mode, C * 131 + npix)
    zd, dad = z.bfloat16().cuda(), da.bfloat16().cuda()
    gd, bd = gamma.float().cuda(), beta.float().cuda()
    a, mean, inv, rmo, rvo = _bn_fwd(ops, zd, gd, bd, rm.float().cuda(), rv.float().cuda(), C, npix)

    # forward reference: torch's training-mode batch_norm in fp64 on the same bf16 z
    rm_ref, rv_ref = rm.clone(), rv.clone()
    y_ref = F.batch_norm(z, rm_ref, rv_ref, gamma, beta, training=True, momentum=MOM, eps=EPS)
    m_ref, var_ref = z.mean(0), z.var(0, unbiased=False)
    inv_ref = 1.0 / torch.sqrt(var_ref + EPS)
    assert float(inv_ref[0]) == 1.0 / math.sqrt(EPS)
    # mean: a blocked reduction (R sum|z| / N).  invstd: M2 is a blocked sum of non-negative terms (R M2); var = M2 / N, + eps, sqrt and the
    # reciprocal add 4 roundings, the square root halves the relative error of the variance: R / 2 + 3u (relative).
    b_mean = R * z.abs().mean(0)
    b_inv = (R / 2 + 3 * U) * inv_ref
    _check("mean", mean, m_ref, b_mean)
    _check("invstd", inv, inv_ref, b_inv)
    # running statistics: (1 - m) r + m stat in fp32 -- the statistic's error times m, 4 roundings of the terms
    _check("running_mean", rmo, rm_ref, MOM * b_mean + 4 * U * ((1 - MOM) * rm.abs() + MOM * m_ref.abs()))
    vu = var_ref * N / (N - 1)
    _check("running_var", rvo, rv_ref, MOM * (R + 2 * U) * vu + 4 * U * ((1 - MOM) * rv.abs() + MOM * vu))
    # a = silu(gamma xhat + beta): y error from the statistics' errors plus 4 roundings; |silu'| <= 1.1; silu evaluated in fp32 within 8u
    # (expf, 1 + e, the division); then one bf16 rounding
    xh = (z - m_ref) * inv_ref
    ey = gamma * (b_mean * inv_ref + xh.abs() * (b_inv / inv_ref)) + 4 * U * ((gamma * xh).abs() + beta.abs())
    a_ref = F.silu(y_ref)
    _check("a", a, a_ref, UBF * a_ref.abs() + (1 + UBF) * (1.1 * ey + 8 * U * a_ref.abs()))

    # backward reference: the batch-statistics backward in fp64 with the device's mean / invstd (the kernel's inputs) as the statistics
    md, isd = mean.double().cpu(), inv.double().cpu()
    xh = (z - md) * isd
    y = gamma * xh + beta
    sg = torch.sigmoid(y)
    ds = sg * (1 + y * (1 - sg))
    gr = da * ds
    db_ref, dg_ref = gr.sum(0), (gr * xh).sum(0)
    dz_ref = gamma * isd * (gr - db_ref / N - xh * dg_ref / N)
    dz, dg, db = _bn_bwd(ops, zd, dad, gd, bd, mean, inv, C, npix)
    # g per element: y within 4u (|gamma xh| + |beta|), |silu''| <= 1/2; silu' in fp32 within 8u s (1 + |y| (1 - s)); the product with da: u
    eg = da.abs() * (0.5 * 4 * U * ((gamma * xh).abs() + beta.abs()) + 8 * U * sg * (1 + y.abs() * (1 - sg))) + U * gr.abs()
    b_db = R * gr.abs().sum(0) + eg.sum(0)
    b_dg = R * (gr * xh).abs().sum(0) + (eg * xh.abs() + 3 * U * (gr * xh).abs()).sum(0)
    _check("dbeta", db, db_ref, b_db)
    _check("dgamma", dg, dg_ref, b_dg)
    inner = gr.abs() + db_ref.abs() / N + (xh * dg_ref).abs() / N
    e_in = eg + (b_db + U * db_ref.abs()) / N + xh.abs() * (b_dg + U * dg_ref.abs()) / N + 2 * U * xh.abs() * dg_ref.abs() / N + 3 * U * inner
    e_dz = (gamma * isd).abs() * e_in + 2 * U * dz_ref.abs()
    _check("dz", dz.reshape(npix, C), dz_ref, UBF * dz_ref.abs() + (1 + UBF) * e_dz)

    # determinism across a grown workspace slot (WS_TRAIN_E: 2 nbx C floats; more channel groups and pixels grow it)
    C2, n2 = C + 256, 4 * npix + 64
    zg, dag = torch.randn(n2, C2, device="cuda").bfloat16(), torch.randn(n2, C2, device="cuda").bfloat16()
    one = torch.ones(C2, device="cuda")

    def grow():
        _, m2, i2 = ops.bn_silu_fwd_bf16(zg, one, one * 0, one * 0, one.clone())
        ops.bn_silu_bwd_bf16(zg, dag, one, one * 0, m2, i2)
    fwd = lambda: torch.cat([t.view(torch.uint8).flatten() for t in _bn_fwd(ops, zd, gd, bd, rm.float().cuda(), rv.float().cuda(), C, npix)])
    _same_thrice("bn forward", fwd, grow)
    bwd = lambda: torch.cat([t.view(torch.uint8).flatten() for t in _bn_bwd(ops, zd, dad, gd, bd, mean, inv, C, npix)])
    _same_thrice("bn backward", bwd, grow)


# ---------------------------------------------------------------------------------------------- SiLU
SILU_SPECIAL = [30.0, -30.0, 100.0, -100.0, BF16_MAX, -BF16_MAX, 0.0, -0.0]


@pytest.mark.parametrize("n", [0, 1, 255, 257, 1 << 20])
def test_silu_fwd_bwd(n):
    """silu(z) = z s, silu'(z) = s (1 + z (1 - s)), s = sigmoid(z), fp32 inside: expf, 1 + e and the division / product keep each within 8u of
    the value (8u s (1 + |z| (1 - s)) for silu'), then one bf16 rounding.  ±inf is left out: silu(-inf) is NaN in torch as well."""
    ops, _ = _ops()
    g = torch.Generator().manual_seed(n)
    z = torch.randn(n, generator=g) * 3
    z[: min(n, len(SILU_SPECIAL))] = torch.tensor(SILU_SPECIAL[: min(n, len(SILU_SPECIAL))])
    z = _bf(z).double()
    da = _bf(torch.randn(n, generator=g)).double()
    zd, dad = z.bfloat16().cuda(), da.bfloat16().cuda()
    c, st = ops.ctx(zd.device), ops._stream()
    a, dz = Guarded((n,), torch.bfloat16), Guarded((n,), torch.bfloat16)
    ops._call("obb_silu_bf16", c, ops._p(zd), ops._p(a.out), n, st)
    ops._call("obb_silu_bwd_bf16", c, ops._p(zd), ops._p(dad), ops._p(dz.out), n, st)
    s = torch.sigmoid(z)
    a_ref = z * s
    ds = s * (1 + z * (1 - s))
    dz_ref = da * ds
    # (bf16's smallest subnormal is 2^-133: a result below half of it rounds to zero, hence the 2^-134 floor)
    _check("silu", a.get("silu"), a_ref, UBF * a_ref.abs() + (1 + UBF) * 8 * U * a_ref.abs() + 2.0 ** -134)
    _check("silu'", dz.get("silu bwd"), dz_ref,
           UBF * dz_ref.abs() + (1 + UBF) * (8 * U * da.abs() * s * (1 + z.abs() * (1 - s))) + 2.0 ** -134)


# ---------------------------------------------------------------------------------------------- bias gradient
def _bias_grad(ops, dyd, npix, cout):
    db = Guarded((cout,), torch.float32)
    ops._call("obb_bias_grad_bf16", ops.ctx(dyd.device), ops._p(dyd), npix, cout, ops._p(db.out), ops._stream())
    return db.get("db")


def _bias_grad_case(ops, dy):
    npix, cout = dy.shape
    dyd = dy.bfloat16().cuda()
    db = _bias_grad(ops, dyd, npix, cout)
    ref, mag = dy.sum(0), dy.abs().sum(0)
    _check(f"bias_grad npix {npix} cout {cout}", db, ref, R * mag)
    big = torch.randn(4 * npix + 64, cout + 64, device="cuda").bfloat16()
    _same_thrice("bias_grad", lambda: _bias_grad(ops, dyd, npix, cout), lambda: ops.bias_grad_bf16(big))
    return float(((db.double().cpu() - ref).abs() / mag).max())


@pytest.mark.parametrize("cout", [1, 12, 64, 80])
@pytest.mark.parametrize("npix", [1, 3, 2 * 52 * 36, 2 * 104 * 104])
def test_bias_grad(npix, cout):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(npix * 7 + cout)
    _bias_grad_case(ops, _bf(torch.randn(npix, cout, generator=g) * 0.1 + torch.randn(cout, generator=g) * 0.05).double())


def test_bias_grad_large_offset():
    """dy ~ N(1, 0.1) over 64 x 104 x 104 pixels: every running sum of a serial fp32 walk over npix / 4 pixels outgrows the bf16 values' spacing
    (6e-6 of sum |dy| in the old kernel); the blocked sums stay within 1e-6."""
    ops, _ = _ops()
    g = torch.Generator().manual_seed(5)
    rel = _bias_grad_case(ops, _bf(torch.randn(64 * 104 * 104, 64, generator=g) * 0.1 + 1.0).double())
    print(f"  bias_grad 64x104x104 x 64, dy ~ N(1, 0.1): max |err| / sum|dy| = {rel:.2e}")


def test_bias_grad_out_length():
    ops, _ = _ops()
    dy = torch.zeros(2, 4, 4, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="entries"):
        ops.bias_grad_bf16(dy, torch.zeros(63, device="cuda"))
    assert ops.bias_grad_bf16(dy, torch.zeros(64, device="cuda")).shape == (64,)
