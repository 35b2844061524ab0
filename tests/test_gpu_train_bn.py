"""f1, training-mode Conv blocks: BatchNorm2d(train) + SiLU forward / backward (csrc/bntrain.hip), the stride-2 3x3 convolution's forward,
dgrad and wgrad (csrc/convgrad.hip), the `Conv` block `train.ConvBN` and the unfolded box branch `train.DetectBoxBranchStep` -- against torch
itself (F.batch_norm(training=True), F.conv2d(stride=2), nn.Module autograd) in fp32 / fp64 at the device's bf16 rounding points."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import loss as ol

import train_steps_ref as TS  # the ConvBN tolerances, shared with the step tests

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.03  # Ultralytics' initialize_weights values


def _q(t):
    """bf16 rounding point with a straight-through gradient."""
    return t + (t.to(torch.bfloat16).float() - t).detach()


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------- BatchNorm(train) + SiLU
def _bn_case(B, H, W, C, seed, mean=None, std=None):
    g = torch.Generator().manual_seed(seed)
    if mean is None:
        mu = torch.randn(C, generator=g) * 0.5
        sd = torch.rand(C, generator=g) * 1.5 + 0.25
    else:
        mu, sd = torch.full((C,), float(mean)), torch.full((C,), float(std))
    z = (torch.randn(B, H, W, C, generator=g) * sd + mu).to(torch.bfloat16)
    gamma = torch.rand(C, generator=g) * 1.5 + 0.25
    beta = torch.randn(C, generator=g) * 0.3
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    return z, gamma, beta, rm, rv, g


BN_CASES = [(16, 104, 104, 128, None, None), (8, 52, 52, 64, None, None), (3, 13, 13, 64, None, None), (16, 104, 104, 64, 8.0, 0.05), (2, 7, 5, 128, None, None)]


@pytest.mark.parametrize("B,H,W,C,mean,std", BN_CASES)
def test_bn_silu_forward(B, H, W, C, mean, std):
    """Batch mean / invstd against fp64 statistics of the same bf16 values, running statistics against F.batch_norm(training=True, momentum=0.03,
    eps=1e-3), a within one bf16 rounding of silu(bn(z)).  The mean = 8, std = 0.05 case would lose the variance to cancellation in a one-pass
    E[z^2] - E[z]^2 (fp32 spacing at 64 is 7.6e-6 against a variance of ~2.5e-3)."""
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    z, gamma, beta, rm, rv, _ = _bn_case(B, H, W, C, B * 7 + H + C, mean, std)
    zd = z.double().reshape(-1, C)
    rm_ref, rv_ref = rm.double().clone(), rv.double().clone()
    y_ref = F.batch_norm(zd, rm_ref, rv_ref, gamma.double(), beta.double(), training=True, momentum=MOM, eps=EPS)
    a_ref = F.silu(y_ref)
    m_ref = zd.mean(0)
    is_ref = 1.0 / torch.sqrt(zd.var(0, unbiased=False) + EPS)

    dev = [t.cuda() for t in (z, gamma, beta, rm, rv)]
    rmd, rvd = dev[3].clone(), dev[4].clone()
    a, m, inv = ops.bn_silu_fwd_bf16(dev[0], dev[1], dev[2], rmd, rvd, EPS, MOM)
    torch.cuda.synchronize()
    em = float(((m.cpu().double() - m_ref).abs() / (m_ref.abs() + zd.std(0))).max())  # fp32 spacing of the mean itself counts
    ei = float(((inv.cpu().double() - is_ref) / is_ref).abs().max())
    erm = float((rmd.cpu().double() - rm_ref).abs().max() / rm_ref.abs().max())
    erv = float(((rvd.cpu().double() - rv_ref) / rv_ref).abs().max())
    ea = ((a.cpu().double().reshape(-1, C) - a_ref).abs() - 2.0 ** -8 * a_ref.abs()).max().item()
    print(f"{B}x{H}x{W}x{C} mean {mean}: |d mean| / (|mean| + std) {em:.2e}, invstd rel {ei:.2e}, running mean {erm:.2e}, running var rel {erv:.2e}, "
          f"a beyond one bf16 rounding {ea:.2e}")
    # measured (MI355X): |d mean| / (|mean| + std) <= 9.1e-8 (the mean-8 case: one fp32 spacing of 8), invstd rel <= 2.1e-7 (also at mean 8,
    # std 0.05), running mean <= 1.2e-7, running var rel <= 1.2e-7, a beyond 2^-8 |a| <= 6.6e-9
    assert em <= 2e-6 and ei <= 2e-5, (em, ei)
    assert erm <= 1e-5 and erv <= 1e-5, (erm, erv)
    assert ea <= 1e-4, ea  # one bf16 rounding of the result (2^-8 relative) plus fp32 evaluation
    rm2, rv2 = dev[3].clone(), dev[4].clone()
    a2, m2, inv2 = ops.bn_silu_fwd_bf16(dev[0], dev[1], dev[2], rm2, rv2, EPS, MOM)
    assert torch.equal(a, a2) and torch.equal(m, m2) and torch.equal(inv, inv2) and torch.equal(rm2, rmd) and torch.equal(rv2, rvd)  # deterministic


@pytest.mark.parametrize("B,H,W,C,mean,std", BN_CASES)
def test_bn_silu_backward(B, H, W, C, mean, std):
    """dz, dgamma, dbeta against fp64 autograd through silu(batch_norm(z, training=True)) on the same bf16 z and da."""
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    z, gamma, beta, rm, rv, g = _bn_case(B, H, W, C, B * 11 + H + C, mean, std)
    da = (torch.randn(B, H, W, C, generator=g) * 0.1).to(torch.bfloat16)
    zd = z.double().reshape(-1, C).requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.batch_norm(zd, None, None, gd, bd, training=True, eps=EPS)
    a_ref = F.silu(y)
    a_ref.backward(da.double().reshape(-1, C))
    # scale of the fp32 sums: sum |g| and sum |g xhat| per channel
    with torch.no_grad():
        s = torch.sigmoid(y)
        gg = da.double().reshape(-1, C) * s * (1 + y * (1 - s))
        xh = (y - bd) / gd
        sg, sgx = gg.abs().sum(0), (gg * xh).abs().sum(0)

    dev = [t.cuda() for t in (z, gamma, beta, rm, rv, da)]
    _, m, inv = ops.bn_silu_fwd_bf16(dev[0], dev[1], dev[2], dev[3], dev[4], EPS, MOM)
    dz, dgam, dbet = ops.bn_silu_bwd_bf16(dev[0], dev[5], dev[1], dev[2], m, inv)
    torch.cuda.synchronize()
    ref_dz = zd.grad
    edz = ((dz.cpu().double().reshape(-1, C) - ref_dz).abs() - 2.0 ** -8 * ref_dz.abs()).max().item() / float(ref_dz.abs().max())
    eg = float(((dgam.cpu().double() - gd.grad).abs() / sgx).max())
    eb = float(((dbet.cpu().double() - bd.grad).abs() / sg).max())
    print(f"{B}x{H}x{W}x{C} mean {mean}: dz beyond one bf16 rounding / max {edz:.2e}, |d dgamma| / sum|g xhat| {eg:.2e}, |d dbeta| / sum|g| {eb:.2e}")
    # measured (MI355X): dz beyond 2^-8 |dz| <= 4.5e-9 of the largest entry (2.8e-7 at mean 8, std 0.05), dgamma / dbeta <= 1.4e-7 of the sums of
    # magnitudes
    assert edz <= 2e-4, edz
    assert eg <= 1e-5 and eb <= 1e-5, (eg, eb)  # fp32 sums in blocks: a few dozen roundings of 6e-8 at most
    dz2, dgam2, dbet2 = ops.bn_silu_bwd_bf16(dev[0], dev[5], dev[1], dev[2], m, inv)
    assert torch.equal(dz, dz2) and torch.equal(dgam, dgam2) and torch.equal(dbet, dbet2)  # deterministic


# ---------------------------------------------------------------------------------------------- stride-2 3x3 convolution
@pytest.mark.parametrize("B,H,W,cin,cout", [(8, 104, 104, 128, 128), (4, 52, 52, 256, 256), (4, 26, 26, 256, 512), (3, 27, 27, 64, 64), (2, 13, 13, 128, 128)])
def test_conv_s2_forward_and_backward(B, H, W, cin, cout):
    """Forward, dgrad (zero insertion + the stride-1 forward kernel) and wgrad of the stride-2 3x3 conv (pad 1, Ho = (H + 1) // 2) against
    F.conv2d(stride=2, padding=1) autograd in fp32 on the same bf16 values: models 3 (at 416 px), 5 and 7 of yolo11s, two odd maps."""
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + H + cin)
    x = (torch.randn((B, cin, H, W), generator=g) * 0.7).bfloat16()
    w = (torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (cin * 9) ** 0.5)).bfloat16()
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    dy = torch.randn((B, cout, Ho, Wo), generator=g).bfloat16()
    xr, wr = x.float().requires_grad_(True), w.float().requires_grad_(True)
    yr = F.conv2d(xr, wr, stride=2, padding=1)
    yr.backward(dy.float())
    xd, dyd, wd = _nhwc(x).cuda(), _nhwc(dy).cuda(), w.float().cuda()
    y = ops.conv_fwd_bf16(xd, ops.conv_pack_bf16(wd, H, W, stride=2), None, cout, 3, stride=2)
    dx = ops.conv_dgrad_s2_bf16(dyd, ops.conv_pack_bf16(wd, H, W, dgrad_form=True), cin, H, W)
    dw = ops.conv_wgrad_bf16(xd, dyd, 3, stride=2)
    assert y.shape == (B, Ho, Wo, cout) and dx.shape == (B, H, W, cin)
    e_y = float((_nchw(y) - yr.detach()).abs().max()) / float(yr.detach().abs().max())
    e_dx = float((_nchw(dx) - xr.grad).abs().max()) / float(xr.grad.abs().max())
    e_dw = float((dw.cpu() - wr.grad).abs().max()) / float(wr.grad.abs().max())
    print(f"{B}x{H}x{W} {cin}->{cout} s2: y max |d| / max {e_y:.2e}, dx {e_dx:.2e} (bf16 outputs), dw {e_dw:.2e}")
    # measured (MI355X): y <= 2.9e-3, dx <= 3.2e-3, dw <= 1.4e-6
    assert e_y <= 6e-3 and e_dx <= 6e-3  # one bf16 rounding of the result (2^-8 relative) + summation order
    assert e_dw <= 2e-5  # fp32 sums of exact bf16 products: summation order only
    assert torch.equal(ops.conv_wgrad_bf16(xd, dyd, 3, stride=2), dw)  # deterministic


# ---------------------------------------------------------------------------------------------- train.ConvBN
def _groups_ref(conv, bn, name, lr, wd):
    groups = [{"params": [conv.weight], "weight_decay": wd}, {"params": [bn.weight], "weight_decay": 0.0}, {"params": [bn.bias], "weight_decay": 0.0}]
    if name == "SGD":
        return torch.optim.SGD(groups, lr=lr, momentum=0.9, nesterov=True, foreach=False)
    return torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), foreach=False)


@pytest.mark.parametrize("B,H,W,c1,c2,k,s", [(4, 26, 26, 64, 64, 1, 1), (2, 52, 52, 64, 128, 3, 1), (2, 27, 27, 128, 128, 3, 2), (2, 52, 52, 128, 128, 3, 2)])
@pytest.mark.parametrize("opt", ["SGD", "AdamW"])
def test_convbn_block_matches_torch_module(B, H, W, c1, c2, k, s, opt):
    """train.ConvBN against nn.Sequential(Conv2d(bias=False), BatchNorm2d(eps=1e-3, momentum=0.03), SiLU()) in .train(): output, dx, dW, dgamma,
    dbeta and the running statistics; the parameters after one optimiser step with the trainer's three groups against torch.optim fed the
    same gradients; fold() through the inference conv + SiLU against the module in .eval()."""
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    import oriented_object_detection_amd.train as TR
    g = torch.Generator().manual_seed(B * 100 + H + c1 + k + s)
    ref = nn.Sequential(nn.Conv2d(c1, c2, k, s, k // 2, bias=False), nn.BatchNorm2d(c2, eps=EPS, momentum=MOM), nn.SiLU()).train()
    with torch.no_grad():
        ref[0].weight.copy_(torch.randn(c2, c1, k, k, generator=g) * (1.5 / (c1 * k * k) ** 0.5))
        ref[1].weight.copy_(torch.rand(c2, generator=g) + 0.5)
        ref[1].bias.copy_(torch.randn(c2, generator=g) * 0.2)
        ref[1].running_mean.copy_(torch.randn(c2, generator=g) * 0.1)
        ref[1].running_var.copy_(torch.rand(c2, generator=g) + 0.5)
    x = torch.randn(B, H, W, c1, generator=g).to(torch.bfloat16)
    Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
    da = (torch.randn(B, Ho, Wo, c2, generator=g) * 0.1).to(torch.bfloat16)

    lr, wd = (0.01 if opt == "SGD" else 0.001), 5e-4
    grp = TR.ParamGroups(opt, lr=lr, momentum=0.9, weight_decay=wd)
    blk = TR.ConvBN(grp, ref[0].weight.detach().cuda(), ref[1].weight.detach().cuda(), ref[1].bias.detach().cuda(), s=s,
                    running_mean=ref[1].running_mean.cuda(), running_var=ref[1].running_var.cuda())
    grp.build()
    a = blk.forward(x.cuda())
    dx = blk.backward(da.cuda())
    torch.cuda.synchronize()

    xr = _nchw(x).requires_grad_(True)
    z = _q(F.conv2d(xr, _q(ref[0].weight), stride=s, padding=k // 2))
    a_ref = _q(ref[2](ref[1](z)))
    a_ref.backward(_nchw(da))
    rel = lambda d, r: float((d - r).abs().max()) / float(r.abs().max())
    e = {"a": rel(_nchw(a), a_ref.detach()), "dx": rel(_nchw(dx), xr.grad), "dW": rel(blk.dw.cpu(), ref[0].weight.grad),
         "dgamma": rel(blk.dgamma.cpu(), ref[1].weight.grad), "dbeta": rel(blk.dbeta.cpu(), ref[1].bias.grad),
         "rmean": rel(blk.running_mean.cpu(), ref[1].running_mean), "rvar": rel(blk.running_var.cpu(), ref[1].running_var)}
    print(f"{B}x{H}x{W} {c1}->{c2} k{k} s{s}: " + ", ".join(f"{n} {v:.2e}" for n, v in e.items()))
    # measured (MI355X, max |d| / max |ref|): a <= 2.5e-3, dx <= 3.4e-3, dW <= 2.0e-3, dgamma / dbeta <= 7.4e-5, running statistics <= 5.2e-7
    assert e["a"] <= TS.CONVBN_TOL["out"] and e["dx"] <= TS.CONVBN_TOL["dx"], e  # bf16 roundings of z and a (forward), of dz and dx (backward)
    assert e["dW"] <= TS.CONVBN_TOL["dW"], e  # the device's bf16 dz vs autograd's exact one
    assert e["dgamma"] <= TS.CONVBN_TOL["dgamma"] and e["dbeta"] <= TS.CONVBN_TOL["dbeta"], e  # fp32 sums of the same g; z differs where its bf16 rounding flipped
    assert e["rmean"] <= TS.CONVBN_TOL["rmean"] and e["rvar"] <= TS.CONVBN_TOL["rvar"], e

    # one optimiser step: the groups' update against torch.optim on the same gradients (group 0 decays, 1 and 2 do not)
    topt = _groups_ref(ref[0], ref[1], opt, lr, wd)
    for p, gr in ((ref[0].weight, blk.dw), (ref[1].weight, blk.dgamma), (ref[1].bias, blk.dbeta)):
        p.grad = gr.cpu().clone()
    topt.step()
    grp.step()
    for p, d in ((ref[0].weight, blk.w), (ref[1].weight, blk.gamma), (ref[1].bias, blk.beta)):
        assert float((d.cpu() - p.detach()).abs().max()) <= TS.PARAM_TOL * max(1.0, float(p.detach().abs().max()))

    # fold(): eval-mode BN folded into the conv, run on the inference conv kernel + SiLU, against the module in .eval()
    ref.eval()
    with torch.no_grad():
        y_eval = ref(_nchw(x))
    wf, bf = blk.fold()
    xd = x.cuda()
    y = ops.silu_bf16(ops.conv_fwd_bf16(xd, ops.conv_pack_bf16(wf.contiguous(), H, W, stride=s), bf.contiguous(), c2, k, stride=s))
    e_fold = rel(_nchw(y), y_eval)
    print(f"  fold: max |d| / max {e_fold:.2e}")
    assert e_fold <= TS.FOLD_RUN_TOL, e_fold  # measured <= 4.3e-3: bf16 folded weights, bf16 z and a


# ---------------------------------------------------------------------------------------------- train.DetectBoxBranchStep
@pytest.mark.parametrize("B,H,W", [(2, 52, 52), (3, 26, 26)])
def test_detect_box_branch_step_matches_autograd(B, H, W):
    """Detect.cv2[i] unfolded -- ConvBN 3x3, ConvBN 3x3, Conv2d 1x1 (+bias) -> DFL loss -- against autograd through the same modules at the same
    bf16 rounding points: loss, every parameter gradient and dx; then a second step() runs on the updated master weights."""
    import oriented_object_detection_amd  # noqa: F401
    import oriented_object_detection_amd.train as TR
    g = torch.Generator().manual_seed(B * 100 + H + 7)
    c = 64
    ws = [torch.randn(c, c, 3, 3, generator=g) * 0.06, torch.randn(c, c, 3, 3, generator=g) * 0.06]
    gs = [torch.rand(c, generator=g) + 0.5 for _ in range(2)]
    bs = [torch.randn(c, generator=g) * 0.1 for _ in range(2)]
    w3, b3 = torch.randn(64, c, 1, 1, generator=g) * 0.15, torch.randn(64, generator=g) * 0.1
    x = torch.randn(B, H, W, c, generator=g).to(torch.bfloat16)
    n = B * H * W
    tgt = torch.rand(n, 4, generator=g) * 14.5
    wgt = torch.rand(n, generator=g) * (torch.rand(n, generator=g) < 0.3)
    tss = float(wgt.sum().clamp_min(1.0))

    P = [nn.Parameter(t.clone()) for t in (ws[0], gs[0], bs[0], ws[1], gs[1], bs[1], w3, b3)]
    xr = _nchw(x).requires_grad_(True)
    a = xr
    for i in range(2):
        wi, gi, bi = P[3 * i: 3 * i + 3]
        z = _q(F.conv2d(a, _q(wi), padding=1))
        a = _q(F.silu(F.batch_norm(z, torch.zeros(c), torch.ones(c), gi, bi, training=True, momentum=MOM, eps=EPS)))
    out = _q(F.conv2d(a, _q(P[6]), P[7]))
    ref_loss = ol.dfl_loss(out.permute(0, 2, 3, 1).reshape(n, 64), tgt, wgt, tss)
    ref_loss.backward()

    st = TR.DetectBoxBranchStep([(ws[i].cuda(), gs[i].cuda(), bs[i].cuda()) for i in range(2)], w3.cuda(), b3.cuda(), "SGD", lr=0.01, momentum=0.9,
                                weight_decay=5e-4)
    loss, dx = st.forward_backward(x.cuda(), tgt.cuda(), wgt.cuda(), tss)
    torch.cuda.synchronize()
    ref_l = float(ref_loss.detach())
    print(f"loss {float(loss):.6f} vs {ref_l:.6f}")
    assert abs(float(loss) - ref_l) <= TS.BOX_STEP_TOL["loss"] * abs(ref_l), (float(loss), ref_l)
    dev = [st.blocks[0].dw, st.blocks[0].dgamma, st.blocks[0].dbeta, st.blocks[1].dw, st.blocks[1].dgamma, st.blocks[1].dbeta, st.dw3, st.db3]
    names = ["dW1", "dgamma1", "dbeta1", "dW2", "dgamma2", "dbeta2", "dW3", "db3"]
    for nm, d, p in zip(names, dev, P):
        e = float((d.cpu() - p.grad).abs().max()) / float(p.grad.abs().max())
        print(f"{nm}: max |d| / max {e:.2e}")
        assert e <= TS.BOX_STEP_TOL["dW"], (nm, e)  # measured <= 4.6e-3: bf16 roundings of the gradient on the way down (one per layer and the BN dz)
    edx = float((_nchw(dx) - xr.grad).abs().max()) / float(xr.grad.abs().max())
    print(f"dx max |d| / max {edx:.2e}")
    assert edx <= TS.BOX_STEP_TOL["dx"], edx  # measured <= 5.8e-3
    # apply this step's update, then a whole step() (forward, backward, gradient average, update) runs on the updated master weights
    w_before = st.blocks[0].w.clone()
    st.groups.step()
    assert not torch.equal(st.blocks[0].w, w_before)
    loss2, _ = st.step(x.cuda(), tgt.cuda(), wgt.cuda(), tss)
    assert torch.isfinite(loss2).all() and float(loss2) != float(loss)


# ---------------------------------------------------------------------------------------------- argument checks
def test_train_bn_argument_checks():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    one = lambda C: torch.ones(C, device="cuda")
    z12 = torch.zeros(2, 4, 4, 12, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.ObbHipError, match="multiple of 8"):
        ops.bn_silu_fwd_bf16(z12, one(12), one(12) * 0, one(12) * 0, one(12))
    with pytest.raises(_lib.ObbHipError, match="multiple of 8"):
        ops.bn_silu_bwd_bf16(z12, z12, one(12), one(12), one(12), one(12))
    z1 = torch.zeros(1, 1, 1, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.ObbHipError, match="npix"):
        ops.bn_silu_fwd_bf16(z1, one(64), one(64) * 0, one(64) * 0, one(64))
    x = torch.zeros(1, 8, 8, 32, dtype=torch.bfloat16, device="cuda")
    dy = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.ObbHipError, match="multiples of 64"):
        ops.conv_wgrad_bf16(x, dy, 3, stride=2)
    # cin = 0 passes `% 64 == 0`: rejected, not a division by zero in the launch plan (real buffers, straight through the C-ABI)
    x64 = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device="cuda")
    dw = torch.zeros(64, 64, 3, 3, device="cuda")
    for name, args in (("obb_conv_wgrad_s2_bf16", (1, 8, 8, 0, 64)), ("obb_conv_wgrad_bf16", (1, 4, 4, 64, 0, 3))):
        with pytest.raises(_lib.ObbHipError, match="at least 64 channels"):
            ops._call(name, ops.ctx(x64.device), ops._p(x64), ops._p(dy), *args, ops._p(dw), ops._stream())
    # one 400-pixel row at stride 2 with 64 channels per side: 3 x 401 + 200 pixels of 128 bytes = 175 KiB, more than a CU's LDS (refused
    # before any buffer is touched)
    with pytest.raises(_lib.ObbHipError, match="does not fit"):
        ops._call("obb_conv_wgrad_s2_bf16", ops.ctx(x64.device), ops._p(x64), ops._p(dy), 1, 2, 400, 64, 64, ops._p(dw), ops._stream())
