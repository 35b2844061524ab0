"""f1, training-mode depthwise 3x3 Conv blocks (csrc/dwgrad.hip, the `act` flag of csrc/bntrain.hip): forward and the fused dx + dw backward per
element against the fp64 references of tests/dw_ref.py (pinned to torch.autograd by test_train_dw_cpu.py) on the bf16-rounded weights, exact
count and impulse cases that a tolerance cannot stand in for, BatchNorm without activation, the argument checks, and `train.DWConvBN` /
`train.ClassBranchPair` against the nn-module reference under the tolerances test_train_dw_cpu.py measures."""
import pytest
import torch
import torch.nn.functional as F

import dw_ref as DR
from bounds import Guarded, U, _check, _same_thrice

pytestmark = pytest.mark.gpu

EPS, MOM = DR.EPS, DR.MOM
BF = 2.0 ** -8  # one bf16 rounding, relative
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]
# nine distinct powers of two, tap (ky, kx) = 2^(3 ky + kx), the last one negated: every sum of a subset is an integer in [-256, 255] whose
# magnitude has at most 8 significant bits -- exact in fp32 whatever the order AND exact in the bf16 the result is stored in
POW2 = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, -256.0]).view(1, 1, 3, 3)


def _ops():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    return ops


def _case(B, H, W, C):
    g = torch.Generator().manual_seed(B * 1000 + H * 37 + W * 5 + C)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    dz = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.5  # fp32 master weights: NOT bf16 values, the kernel rounds them
    return x, dz, w


def _bwd(O, xd, dd, wd, shape, dx=True, dw=True):
    """-> (Guarded dx, Guarded dw) after one obb_dwconv3_bwd_bf16; a half that is off is passed as NULL and its buffer handed back untouched."""
    gx, gw = Guarded(shape, torch.bfloat16), Guarded((shape[3], 1, 3, 3), torch.float32)
    O.dwconv3_bwd(xd, dd, wd, gx.out if dx else None, gw.out if dw else None)
    return gx, gw


# ---------------------------------------------------------------------------------------------- per-element bounds
@pytest.mark.parametrize("B,H,W,C", DR.DW_SHAPES)
def test_dwconv3_forward_and_fused_backward(B, H, W, C):
    """z and dx within one bf16 rounding of the result plus 10 fp32 roundings of the sum of magnitudes (9 products, at most 9 additions, one of
    slack); dw within (L + 2) fp32 roundings of it, L the launcher's own addition chain at this shape; the references use the bf16-rounded
    weights.  The forms with one output NULL are bit-equal to the fused call and leave the other buffer untouched; dw is bit-identical on a second
    call and after the workspace slot has grown."""
    ops = _ops()
    O = torch.ops.obbhip
    what = f"{B}x{H}x{W}x{C}"
    x, dz, w = _case(B, H, W, C)
    wq = DR.bf16(w).double()
    L = ops.dwconv3_bwd_geometry(B, H, W, C)[3]
    assert L <= 96
    z_ref, z_S = DR.dw_fwd_ref(x.double(), wq), DR.dw_fwd_ref(x.double().abs(), wq.abs())
    (dx_ref, dw_ref), (dx_S, dw_S) = DR.dw_bwd_ref(x.double(), dz.double(), wq), DR.dw_bwd_ref(x.double().abs(), dz.double().abs(), wq.abs())

    xd, dd, wd = x.cuda(), dz.cuda(), w.cuda()
    gz = Guarded((B, H, W, C), torch.bfloat16)
    O.dwconv3_fwd(xd, wd, gz.out)
    z = gz.get(what + " z")
    _check(what + " z", z, z_ref, BF * z_ref.abs() + 10 * U * z_S)
    assert torch.equal(ops.dwconv3_fwd_bf16(xd, wd), z), what + ": second forward differs"

    gx, gw = _bwd(O, xd, dd, wd, (B, H, W, C))
    dx, dw = gx.get(what + " dx"), gw.get(what + " dw")
    _check(what + " dx", dx, dx_ref, BF * dx_ref.abs() + 10 * U * dx_S)
    _check(what + f" dw (L = {L})", dw, dw_ref, (L + 2) * U * dw_S)

    gx1, gw1 = _bwd(O, xd, dd, wd, (B, H, W, C), dx=False)
    assert torch.equal(gw1.get(what + " dw alone"), dw), what + ": dw alone is not bit-equal to the fused dw"
    assert bool((gx1.raw == 0xFF).all()), what + ": dx written although NULL"
    gx2, gw2 = _bwd(O, xd, dd, wd, (B, H, W, C), dw=False)
    assert torch.equal(gx2.get(what + " dx alone"), dx), what + ": dx alone is not bit-equal to the fused dx"
    assert bool((gw2.raw == 0xFF).all()), what + ": dw written although NULL"
    only_dw = ops.dwconv3_bwd_bf16(xd, dd, wd, need_dx=False)
    assert only_dw[0] is None and torch.equal(only_dw[1], dw)

    # 8 x 10 x 40 runs on 8 lane rows: 400 slabs of 9 x 512 floats, more than any shape above asks for (the values do not matter)
    big = [torch.zeros(8, 40, 40, 512, dtype=torch.bfloat16, device="cuda")] * 2 + [torch.zeros(512, 1, 3, 3, device="cuda")]
    _same_thrice(what + " dw", lambda: ops.dwconv3_bwd_bf16(xd, dd, wd)[1], lambda: ops.dwconv3_bwd_bf16(*big))


# ---------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("B,H,W,C", DR.DW_SHAPES)
def test_dwconv3_counts_are_exact(B, H, W, C):
    """x = 1, dz = 1: dw[c,ky,kx] is the number of pixels whose tap (ky, kx) lies in the map, B (H - |ky - 1|) (W - |kx - 1|), exactly (below
    2^24); the forward of x = 1 under nine distinct power-of-two taps (POW2) is, at every pixel, the exact sum of the taps in range."""
    ops = _ops()
    one = torch.ones(B, H, W, C, dtype=torch.bfloat16, device="cuda")
    w = POW2.expand(C, 1, 3, 3).contiguous()
    _, dw = ops.dwconv3_bwd_bf16(one, one, w.cuda())
    want = torch.tensor([[B * (H - abs(ky - 1)) * (W - abs(kx - 1)) for kx in range(3)] for ky in range(3)], dtype=torch.float32)
    assert float(want.max()) < 2 ** 24
    assert torch.equal(dw.cpu(), want.view(1, 1, 3, 3).expand(C, 1, 3, 3)), (dw[0, 0].cpu(), want)
    z = ops.dwconv3_fwd_bf16(one, w.cuda()).cpu().double()
    assert torch.equal(z, DR.dw_fwd_ref(torch.ones(B, H, W, C, dtype=torch.float64), w.double()))


def _impulse_pixels(H, W, rows):
    """The four corners, an edge midpoint, the centre, and every column of the first and the last row of every stripe: with one lane run per
    (stripe, column) these are the first and the last pixel of every stripe and of every lane run."""
    px = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, W // 2)}
    for i0 in range(0, H, rows):
        for i in (i0, min(i0 + rows, H) - 1):
            px.update((i, j) for j in range(W))
    return sorted(px)


@pytest.mark.parametrize("B,H,W,C", DR.DW_SHAPES)
def test_dwconv3_impulses_are_exact(B, H, W, C):
    """dz one-hot at pixel p (random x): dw[c,ky,kx] is bit-equal to x[p + (ky - 1, kx - 1)], 0 outside the map -- one pixel per channel and call
    (channels are independent), every image in turn.  x one-hot under nine distinct power-of-two taps: z bit-equal to the reference (a
    transposed or flipped kernel, an H / W swap); the same for dx from a one-hot dz."""
    ops = _ops()
    rows = ops.dwconv3_bwd_geometry(B, H, W, C)[0]
    x, _, _ = _case(B, H, W, C)
    xd, xp = x.cuda(), F.pad(x.float(), (0, 0, 1, 1, 1, 1))
    wz = torch.zeros(C, 1, 3, 3, device="cuda")
    pix = _impulse_pixels(H, W, rows)
    ch = torch.arange(C)
    for n0 in range(0, len(pix), C):
        part = pix[n0:n0 + C]
        k = len(part)
        b = (torch.arange(k) + n0) % B
        pi, pj = torch.tensor([p[0] for p in part]), torch.tensor([p[1] for p in part])
        dz = torch.zeros(B, H, W, C)
        dz[b, pi, pj, ch[:k]] = 1.0
        _, dw = ops.dwconv3_bwd_bf16(xd, dz.to(torch.bfloat16).cuda(), wz)
        want = torch.zeros(C, 1, 3, 3)
        for ky, kx in TAPS:
            want[:k, 0, ky, kx] = xp[b, pi + ky, pj + kx, ch[:k]]  # padded index: p + (ky - 1, kx - 1) + 1
        assert torch.equal(dw.cpu(), want), f"{B}x{H}x{W}x{C}: pixels {part[0]}..{part[-1]}"

    w = POW2.expand(C, 1, 3, 3).contiguous()
    for (pi, pj) in [(0, 0), (H - 1, W - 1), (H // 2, W // 2), (H - 1, 0), (min(rows, H) - 1, W // 2), (min(rows, H - 1), W - 1)]:
        hot = torch.zeros(B, H, W, C, dtype=torch.float64)
        hot[B - 1, pi, pj, :] = 1.0
        hb = hot.to(torch.bfloat16).cuda()
        assert torch.equal(ops.dwconv3_fwd_bf16(hb, w.cuda()).cpu().double(), DR.dw_fwd_ref(hot, w.double())), (pi, pj, "z")
        dx, _ = ops.dwconv3_bwd_bf16(hb, hb, w.cuda())
        assert torch.equal(dx.cpu().double(), DR.dw_bwd_ref(hot, hot, w.double())[0]), (pi, pj, "dx")


# ---------------------------------------------------------------------------------------------- BatchNorm without activation
def _bn_case(C, B, H, W):
    g = torch.Generator().manual_seed(C * 7 + B + H + W)
    z = (torch.randn(B, H, W, C, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.25) + torch.randn(C, generator=g) * 0.5).to(torch.bfloat16)
    gamma, beta = torch.rand(C, generator=g) * 1.5 + 0.25, torch.randn(C, generator=g) * 0.3
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    da = (torch.randn(B, H, W, C, generator=g) * 0.1).to(torch.bfloat16)
    return z, gamma, beta, rm, rv, da


@pytest.mark.parametrize("C,B,H,W", [(128, 2, 13, 13), (256, 3, 4, 4), (24, 2, 13, 9)])
def test_bn_without_activation(C, B, H, W):
    """obb_bn_fwd_bf16 / obb_bn_bwd_bf16 with act = 0 against bn_ref (forward) and fp64 autograd through it (backward), under the bounds
    test_gpu_train_bn.py holds the SiLU form to; act = 1 through the new entry points is bit-equal to the old ones."""
    ops = _ops()
    z, gamma, beta, rm, rv, da = _bn_case(C, B, H, W)
    zd = z.double().reshape(-1, C).requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a_ref = DR.bn_ref(zd, gd, bd, EPS, False)
    a_ref.backward(da.double().reshape(-1, C))
    rm_ref, rv_ref = rm.double().clone(), rv.double().clone()
    F.batch_norm(zd.detach(), rm_ref, rv_ref, None, None, training=True, momentum=MOM, eps=EPS)
    with torch.no_grad():
        m_ref, sd = zd.mean(0), zd.std(0)
        is_ref = 1.0 / torch.sqrt(zd.var(0, unbiased=False) + EPS)
        gg = da.double().reshape(-1, C)
        sg, sgx = gg.abs().sum(0), (gg * (zd - m_ref) * is_ref).abs().sum(0)

    dev = [t.cuda() for t in (z, gamma, beta, rm, rv, da)]
    rmd, rvd = dev[3].clone(), dev[4].clone()
    a, m, inv = ops.bn_fwd_bf16(dev[0], dev[1], dev[2], rmd, rvd, EPS, MOM, act=False)
    dz, dgam, dbet = ops.bn_bwd_bf16(dev[0], dev[5], dev[1], dev[2], m, inv, act=False)
    torch.cuda.synchronize()
    em = float(((m.cpu().double() - m_ref).abs() / (m_ref.abs() + sd)).max())
    ei = float(((inv.cpu().double() - is_ref) / is_ref).abs().max())
    erm = float((rmd.cpu().double() - rm_ref).abs().max() / rm_ref.abs().max())
    erv = float(((rvd.cpu().double() - rv_ref) / rv_ref).abs().max())
    ea = ((a.cpu().double().reshape(-1, C) - a_ref.detach()).abs() - BF * a_ref.detach().abs()).max().item()
    edz = ((dz.cpu().double().reshape(-1, C) - zd.grad).abs() - BF * zd.grad.abs()).max().item() / float(zd.grad.abs().max())
    eg = float(((dgam.cpu().double() - gd.grad).abs() / sgx).max())
    eb = float(((dbet.cpu().double() - bd.grad).abs() / sg).max())
    print(f"{B}x{H}x{W}x{C} act 0: mean {em:.2e}, invstd {ei:.2e}, running {erm:.2e} / {erv:.2e}, a beyond a rounding {ea:.2e}, dz {edz:.2e}, dgamma {eg:.2e}, "
          f"dbeta {eb:.2e}")
    assert em <= 2e-6 and ei <= 2e-5, (em, ei)
    assert erm <= 1e-5 and erv <= 1e-5, (erm, erv)
    assert ea <= 1e-4, ea
    assert edz <= 2e-4, edz
    assert eg <= 1e-5 and eb <= 1e-5, (eg, eb)

    r1, v1, r2, v2 = dev[3].clone(), dev[4].clone(), dev[3].clone(), dev[4].clone()
    old = ops.bn_silu_fwd_bf16(dev[0], dev[1], dev[2], r1, v1, EPS, MOM)
    new = ops.bn_fwd_bf16(dev[0], dev[1], dev[2], r2, v2, EPS, MOM, act=True)
    assert all(torch.equal(p, q) for p, q in zip(old + (r1, v1), new + (r2, v2))), "act = 1 forward differs from obb_bn_silu_fwd_bf16"
    oldb = ops.bn_silu_bwd_bf16(dev[0], dev[5], dev[1], dev[2], old[1], old[2])
    newb = ops.bn_bwd_bf16(dev[0], dev[5], dev[1], dev[2], new[1], new[2], act=True)
    assert all(torch.equal(p, q) for p, q in zip(oldb, newb)), "act = 1 backward differs from obb_bn_silu_bwd_bf16"
    assert not torch.equal(new[0], a)


# ---------------------------------------------------------------------------------------------- argument checks
def test_dw_argument_checks():
    ops = _ops()
    from oriented_object_detection_amd import _lib
    zb = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    x, w, dw = zb(1, 4, 4, 8), torch.zeros(8, 1, 3, 3, device="cuda"), torch.zeros(8, 1, 3, 3, device="cuda")
    c, P, S = ops.ctx(), ops._p, ops._stream
    with pytest.raises(_lib.ObbHipError, match="NULL"):
        ops._call("obb_dwconv3_fwd_bf16", c, P(x), P(None), 1, 4, 4, 8, P(zb(1, 4, 4, 8)), S())
    with pytest.raises(_lib.ObbHipError, match="NULL"):
        ops._call("obb_dwconv3_bwd_bf16", c, P(x), P(None), P(w), 1, 4, 4, 8, P(zb(1, 4, 4, 8)), P(dw), S())
    with pytest.raises(_lib.ObbHipError, match="NULL"):  # dw asked for without x
        ops._call("obb_dwconv3_bwd_bf16", c, P(None), P(x), P(w), 1, 4, 4, 8, P(None), P(dw), S())
    with pytest.raises(_lib.ObbHipError, match="both NULL"):
        ops._call("obb_dwconv3_bwd_bf16", c, P(x), P(x), P(w), 1, 4, 4, 8, P(None), P(None), S())
    x12, w12 = zb(1, 4, 4, 12), torch.zeros(12, 1, 3, 3, device="cuda")
    with pytest.raises(_lib.ObbHipError, match="multiple of 8"):
        ops.dwconv3_fwd_bf16(x12, w12)
    with pytest.raises(_lib.ObbHipError, match="multiple of 8"):
        ops.dwconv3_bwd_bf16(x12, x12, w12)
    with pytest.raises(_lib.ObbHipError, match="at least 1"):
        ops._call("obb_dwconv3_fwd_bf16", c, P(x), P(w), 0, 4, 4, 8, P(zb(1, 4, 4, 8)), S())
    with pytest.raises(_lib.ObbHipError, match="at least 1"):
        ops._call("obb_dwconv3_bwd_bf16", c, P(x), P(x), P(w), 0, 4, 4, 8, P(zb(1, 4, 4, 8)), P(dw), S())
    one = torch.ones(8, device="cuda")
    with pytest.raises(_lib.ObbHipError, match="act = 2"):
        ops._call("obb_bn_fwd_bf16", c, P(x), 16, 8, P(one), P(one), 1e-3, 0.03, P(one.clone()), P(one.clone()), P(one.clone()), P(one.clone()), P(zb(1, 4, 4, 8)), 2, S())
    with pytest.raises(_lib.ObbHipError, match="multiple of 8"):
        ops.bn_fwd_bf16(x12, torch.ones(12, device="cuda"), torch.ones(12, device="cuda"), torch.ones(12, device="cuda"), torch.ones(12, device="cuda"), act=False)
    with pytest.raises(ValueError, match=r"\[C,1,3,3\]"):
        ops.dwconv3_fwd_bf16(x, torch.zeros(8, 3, 3, device="cuda"))


# ---------------------------------------------------------------------------------------------- train.DWConvBN, train.ClassBranchPair
def _dev_args(blk):
    return tuple(t.clone().cuda() for t in blk.init)


def _nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _block_results(tag, blk):
    return {f"{tag}dW": blk.dw, f"{tag}dgamma": blk.dgamma, f"{tag}dbeta": blk.dbeta, f"{tag}rmean": blk.running_mean, f"{tag}rvar": blk.running_var}


def _assert_within_2e(what, got, plain, rounded):
    """Per tensor: e = max |rounded - plain| / max |plain| (the figure test_train_dw_cpu.py keeps in a band), device within 2 e of plain."""
    assert set(got) == set(plain), set(got) ^ set(plain)
    d = {n: DR.rel_dist(got[n].cpu(), plain[n]) for n in plain}
    e = {n: DR.rel_dist(rounded[n], plain[n]) for n in plain}
    print(f"{what}: " + ", ".join(f"{n} {d[n]:.2e} (e {e[n]:.2e})" for n in plain))
    for n in plain:
        assert d[n] <= 2 * e[n], (what, n, d[n], e[n])


@pytest.mark.parametrize("B,H,W,C,act", [(2, 26, 26, 128, True), (2, 13, 13, 128, False)])
def test_dwconvbn_block_matches_torch_modules(B, H, W, C, act):
    """train.DWConvBN against Conv2d(C, C, 3, 1, 1, groups=C, bias=False) -> BatchNorm2d(eps 1e-3, momentum 0.03) [-> SiLU] in .train(): out, dx,
    dW, dgamma, dbeta and the running statistics, each within twice the rounded-against-plain figure of the reference itself."""
    _ops()
    import oriented_object_detection_amd.train as TR
    case = DR.dwbn_case(B, H, W, C, act)
    ref, x, da = case
    grp = TR.ParamGroups("SGD", lr=0.01, momentum=0.9, weight_decay=5e-4)
    a = _dev_args(ref)
    blk = TR.DWConvBN(grp, a[0], a[1], a[2], act, a[3], a[4], EPS, MOM)
    grp.build()
    out = blk.forward(x.cuda())
    dx = blk.backward(da.cuda())
    torch.cuda.synchronize()
    got = {"out": _nchw(out), "dx": _nchw(dx), **_block_results("", blk)}
    _assert_within_2e(f"DWConvBN {B}x{H}x{W}x{C} act {act}", got, DR.run_dwbn(case, False), DR.run_dwbn(case, True))
    wf, bf = blk.fold()
    f = blk.gamma / torch.sqrt(blk.running_var + EPS)
    assert wf.shape == (C, 1, 3, 3) and torch.equal(wf, blk.w * f.view(-1, 1, 1, 1)) and torch.equal(bf, blk.beta - blk.running_mean * f)


def test_class_branch_pair_matches_torch_modules_and_sgd():
    """train.ClassBranchPair (DWConv 3x3 -> Conv 1x1, 128 -> 64 at 26 x 26) against the four-module stack, then one step of the three groups
    against torch.optim.SGD fed the same gradients."""
    _ops()
    import oriented_object_detection_amd.train as TR
    B, H, W, c1, c2 = 2, 26, 26, 128, 64
    case = DR.pair_case(B, H, W, c1, c2)
    rdw, rpw, x, da = case
    lr, wd = 0.01, 5e-4
    grp = TR.ParamGroups("SGD", lr=lr, momentum=0.9, weight_decay=wd)
    pair = TR.ClassBranchPair(grp, _dev_args(rdw), _dev_args(rpw), EPS, MOM)
    grp.build()
    out = pair.forward(x.cuda())
    dx = pair.backward(da.cuda())
    torch.cuda.synchronize()
    got = {"out": _nchw(out), "dx": _nchw(dx), **_block_results("dw.", pair.dw), **_block_results("pw.", pair.pw)}
    _assert_within_2e("ClassBranchPair", got, DR.run_pair(case, False), DR.run_pair(case, True))

    blocks = [(rdw, pair.dw), (rpw, pair.pw)]
    for r, _ in blocks:
        r.reset()
        r.seq.float()
    params = lambda r: (r.seq[0].weight, r.seq[1].weight, r.seq[1].bias)
    topt = torch.optim.SGD([{"params": [params(r)[k] for r, _ in blocks], "weight_decay": wd if k == 0 else 0.0} for k in range(3)], lr=lr, momentum=0.9,
                           nesterov=True, foreach=False)
    for r, blk in blocks:
        for p, gr in zip(params(r), (blk.dw, blk.dgamma, blk.dbeta)):
            p.grad = gr.cpu().clone()
    topt.step()
    grp.step()
    for r, blk in blocks:
        for p, dv in zip(params(r), (blk.w, blk.gamma, blk.beta)):
            assert float((dv.cpu() - p.detach()).abs().max()) <= 2e-6 * max(1.0, float(p.detach().abs().max()))
