"""f1, C2PSA attention in training mode (csrc/attngrad.hip, obb_add_bf16 of csrc/routegrad.hip, `train.Attention` / `train.PSABlock`): the
core's forward and backward per element against the fp64 references of tests/attn_ref.py under its a-priori bounds (which test_train_attn_cpu.py
shows to catch the mistakes they are there for), exact cases that no tolerance can stand in for, dv_add, reproducibility, the argument checks,
the bf16 add, ConvBN(act=False) and the assembled blocks against the nn-module reference."""
import pytest
import torch

import attn_ref as AR
import block_ref as BR
import dw_ref as DR
import train_steps_ref as TS  # the fold and optimiser-step tolerances, shared with the step tests
from bounds import Guarded, _check, _same_thrice

pytestmark = pytest.mark.gpu

EPS, MOM = DR.EPS, DR.MOM


def _ops():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    return ops


def _fwd(qkv, nh):
    """-> (out, lse) through Guarded buffers"""
    B, N = qkv.shape[0], qkv.shape[1]
    go, gl = Guarded((B, N, nh * 64), torch.bfloat16), Guarded((B, nh, N), torch.float32)
    torch.ops.obbhip.attn_fwd(qkv, nh, go.out, gl.out)
    what = f"N {N} nh {nh} B {B}"
    return go.get(what + " out"), gl.get(what + " lse")


def _bwd(qkv, out, lse, dout, nh, dv_add=None):
    g = Guarded(tuple(qkv.shape), torch.bfloat16)
    torch.ops.obbhip.attn_bwd(qkv, out, lse, dout, dv_add, nh, g.out)
    return g.get(f"N {qkv.shape[1]} nh {nh} B {qkv.shape[0]} dqkv")


# ---------------------------------------------------------------------------------------------- per-element bounds
@pytest.mark.parametrize("nh,B", AR.HEADS)
@pytest.mark.parametrize("N", AR.NS)
def test_attention_core_per_element(N, nh, B):
    """out and lse against the fp64 forward; dq, dk, dv against the fp64 backward OF THE SAME INPUTS (the device's own out and lse), each element
    under its a-priori bound; dv_add under the same bound, and dv_add = 0 bit-equal to the NULL form."""
    _ops()
    what = f"N {N} nh {nh} B {B}"
    qkv, dout, dv_add = AR.core_case(N, nh, B)
    o_ref, l_ref = AR.attn_fwd_ref(qkv, nh)
    Eo, El = AR.attn_fwd_bounds(qkv, nh)
    qd, dd, ad = qkv.cuda(), dout.cuda(), dv_add.cuda()
    out, lse = _fwd(qd, nh)
    _check(what + " out", out, o_ref, Eo)
    _check(what + " lse", lse, l_ref, El)

    oc, lc = out.cpu(), lse.cpu()
    dqkv = _bwd(qd, out, lse, dd, nh)
    ref, E = AR.attn_bwd_ref(qkv, oc, lc, dout, nh, parts=True), AR.attn_bwd_bounds(qkv, oc, lc, dout, nh, parts=True)
    for name, got, r, e in zip(("dq", "dk", "dv"), AR.split(dqkv.cpu(), nh), ref, E):
        _check(f"{what} {name}", got, r, e)

    dqkv_a = _bwd(qd, out, lse, dd, nh, ad)
    ref_a, E_a = AR.attn_bwd_ref(qkv, oc, lc, dout, nh, dv_add), AR.attn_bwd_bounds(qkv, oc, lc, dout, nh, dv_add)
    _check(what + " dqkv with dv_add", dqkv_a, ref_a, E_a)
    assert torch.equal(dqkv_a[..., :nh * 64], dqkv[..., :nh * 64]), what + ": dv_add changed dq / dk"
    assert torch.equal(_bwd(qd, out, lse, dd, nh, torch.zeros_like(ad)), dqkv), what + ": dv_add = 0 is not bit-equal to NULL"


# ---------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("zero", ["q", "k"])
def test_uniform_attention_is_exact(zero):
    """q = 0 (N = 16): P = 1 / 16 exactly, out the exact mean of v, dv = (1 / 16) sum dout exactly, dk exactly 0.  k = 0: dq exactly 0 (and out, dv as
    before: S = 0 either way)."""
    _ops()
    N, nh, B = 16, 2, 2
    qkv, dout = AR.uniform_case(N, nh, B, zero)
    out, lse = _fwd(qkv.cuda(), nh)
    _, _, v = AR.split(qkv.double(), nh)
    (do,) = AR.split(dout.double(), nh, (64,))
    mean = v.mean(2, keepdim=True).expand_as(v)
    assert torch.equal(AR.split(out.cpu().double(), nh, (64,))[0], mean), "out is not the exact mean"  # (multiples of 1 / 16 below 8: bf16 values)
    dq, dk, dv = AR.split(_bwd(qkv.cuda(), out, lse, dout.cuda(), nh).cpu().double(), nh)
    assert torch.equal(dv, (do.sum(2, keepdim=True) / 16).expand_as(do).to(torch.bfloat16).double()), "dv is not the exact (1 / 16) sum of dout"
    assert float((do.sum(2) / 16 - (do.sum(2) / 16).to(torch.bfloat16).double()).abs().max()) == 0  # ... which is itself a bf16 value
    assert bool(((dk if zero == "q" else dq) == 0).all()), f"{'dk' if zero == 'q' else 'dq'} is not exactly 0"


@pytest.mark.parametrize("N", [16, 17, 169])
def test_one_hot_attention_is_exact(N):
    """Query n matches key pi(n) alone: out[n] bit-equal to v[pi(n)], dv[pi(n)] bit-equal to dout[n], dq and dk exactly 0 (dP = D exactly on
    small integers).  Every transpose or index exchange fails here, and at N = 17 and 169 so does a padded query that leaks into dk / dv."""
    _ops()
    nh, B = 3, 2
    qkv, dout, pi = AR.onehot_case(N, nh, B)
    out, lse = _fwd(qkv.cuda(), nh)
    q, k, v = AR.split(qkv.double(), nh)
    (do,) = AR.split(dout.double(), nh, (64,))
    idx = pi.unsqueeze(-1).expand(B, nh, N, 64)
    assert torch.equal(AR.split(out.cpu().double(), nh, (64,))[0], v.gather(2, idx)), "out[n] != v[pi(n)]"
    assert torch.equal(lse.cpu().double(), torch.full((B, nh, N), 8192.0 * AR.SCALE).float().double()), "lse != the matched score"
    dq, dk, dv = AR.split(_bwd(qkv.cuda(), out, lse, dout.cuda(), nh).cpu().double(), nh)
    assert torch.equal(dv.gather(2, idx), do), "dv[pi(n)] != dout[n]"
    assert bool((dq == 0).all()) and bool((dk == 0).all()), "dq / dk not exactly 0"


# ---------------------------------------------------------------------------------------------- reproducibility, arguments
def test_backward_is_bit_reproducible():
    ops = _ops()
    qkv, dout, dv_add = AR.core_case(169, 2, 2)
    qd, dd, ad = qkv.cuda(), dout.cuda(), dv_add.cuda()
    out, lse = ops.attn_fwd_bf16(qd, 2)
    big_q = torch.zeros(8, 192, 6 * 128, dtype=torch.bfloat16, device="cuda")
    big_o, big_l = ops.attn_fwd_bf16(big_q, 6)
    _same_thrice("dqkv", lambda: ops.attn_bwd_bf16(qd, out, lse, dd, 2, ad), lambda: ops.attn_bwd_bf16(big_q, big_o, big_l, big_o, 6))
    o2, l2 = ops.attn_fwd_bf16(qd, 2)
    assert torch.equal(o2, out) and torch.equal(l2, lse)


def test_attn_argument_checks():
    ops = _ops()
    from oriented_object_detection_amd import _lib
    c, P, S = ops.ctx(), ops._p, ops._stream
    zb = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    q, o, l = zb(1, 16, 128), zb(1, 16, 64), torch.zeros(1, 1, 16, device="cuda")
    go, gl, gd = Guarded((1, 16, 64), torch.bfloat16), Guarded((1, 1, 16), torch.float32), Guarded((1, 16, 128), torch.bfloat16)
    for N, nh, B, pat in ((0, 1, 1, "tokens"), (193, 1, 1, "tokens"), (16, 0, 1, "at least 1"), (16, 1, 0, "at least 1")):
        with pytest.raises(_lib.ObbHipError, match=pat):
            ops._call("obb_attn_fwd_bf16", c, P(q), B, N, nh, P(go.out), P(gl.out), S())
        with pytest.raises(_lib.ObbHipError, match=pat):
            ops._call("obb_attn_bwd_bf16", c, P(q), P(o), P(l), P(o), P(None), B, N, nh, P(gd.out), S())
    with pytest.raises(_lib.ObbHipError, match="NULL"):
        ops._call("obb_attn_fwd_bf16", c, P(q), 1, 16, 1, P(go.out), P(None), S())
    for k in range(4):  # each required input in turn
        a = [P(q), P(o), P(l), P(o)]
        a[k] = P(None)
        with pytest.raises(_lib.ObbHipError, match="NULL"):
            ops._call("obb_attn_bwd_bf16", c, *a, P(None), 1, 16, 1, P(gd.out), S())
    with pytest.raises(_lib.ObbHipError, match="NULL"):
        ops._call("obb_attn_bwd_bf16", c, P(q), P(o), P(l), P(o), P(None), 1, 16, 1, P(None), S())
    with pytest.raises(ValueError, match="nh \\* 128"):  # a wrong channel count
        ops.attn_fwd_bf16(zb(1, 16, 192), 1)
    with pytest.raises(ValueError, match="nh \\* 128"):
        ops.attn_fwd_bf16(q, 0)
    with pytest.raises(ValueError, match="nh \\* 64"):
        ops.attn_bwd_bf16(q, zb(1, 16, 128), l, o, 1)
    with pytest.raises(ValueError, match="do not belong"):
        ops.attn_bwd_bf16(q, o, torch.zeros(1, 1, 15, device="cuda"), o, 1)
    with pytest.raises(_lib.ObbHipError, match="tokens"):
        ops.attn_fwd_bf16(zb(1, 193, 128), 1)
    torch.cuda.synchronize()
    for g in (go, gl, gd):
        assert bool((g.raw == 0xFF).all()), "a rejected call wrote to its output"


def test_add_bf16():
    ops = _ops()
    from oriented_object_detection_amd import _lib
    g = torch.Generator().manual_seed(3)
    for n in (8, 8 * 1000 + 8):
        a = (torch.randn(n, generator=g) * 3).to(torch.bfloat16).cuda()
        b = (torch.randn(n, generator=g) * 3).to(torch.bfloat16).cuda()
        want = (a.float() + b.float()).bfloat16()
        go = Guarded((n,), torch.bfloat16)
        torch.ops.obbhip.add_bf16(a, b, go.out)
        assert torch.equal(go.get(f"add n = {n}"), want)
        ga = Guarded((n,), torch.bfloat16, init=a)
        assert ops.add_bf16(ga.out, b, out=ga.out) is ga.out
        assert torch.equal(ga.get(f"add in place n = {n}"), want)
    x12 = torch.zeros(12, dtype=torch.bfloat16, device="cuda")
    g12 = Guarded((12,), torch.bfloat16)
    with pytest.raises(_lib.ObbHipError, match="multiple of 8"):
        ops.add_bf16(x12, x12, out=g12.out)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.add_bf16(x12, torch.zeros(16, dtype=torch.bfloat16, device="cuda"))
    torch.cuda.synchronize()
    assert bool((g12.raw == 0xFF).all())


# ---------------------------------------------------------------------------------------------- ConvBN(act=False)
def _dev_args(blk):
    return tuple(t.clone().cuda() for t in blk.init)


def _nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _block_results(tag, blk, inv=None):
    r = {f"{tag}dW": blk.dw, f"{tag}dgamma": blk.dgamma, f"{tag}dbeta": blk.dbeta, f"{tag}rmean": blk.running_mean, f"{tag}rvar": blk.running_var}
    return r if inv is None else {n: t[inv] for n, t in r.items()}


def _assert_within_2e(what, got, plain, rounded):
    """Per tensor: e = the rounded reference's distance from plain (attn_ref.block_dist, the figure test_train_attn_cpu.py prints), device within
    2 e of plain."""
    d, e = AR.block_dist(got, plain), AR.block_dist(rounded, plain)
    assert set(got) == set(d), set(got) ^ set(d)
    print(f"{what}: " + ", ".join(f"{n} {d[n]:.2e} (e {e[n]:.2e})" for n in d))
    for n in d:
        assert d[n] <= 2 * e[n], (what, n, d[n], e[n])


def test_convbn_without_activation():
    """train.ConvBN(act=False) (1x1, 128 -> 256 at 2 x 13 x 13: attn.qkv's shape) against Conv2d -> BatchNorm2d in .train() under ConvBN's
    criterion; ConvBN(act=True) bit-equal to a block built without the keyword."""
    _ops()
    import oriented_object_detection_amd.train as TR
    B, H, W, c1, c2 = 2, 13, 13, 128, 256
    g = torch.Generator().manual_seed(77)
    ref = DR.RefBlock(g, c1, c2, 1, 1, False)
    x, da = torch.randn(B, H, W, c1, generator=g).to(torch.bfloat16), DR._grad_in(g, B, H, W, c2)
    grp = TR.ParamGroups()
    a = _dev_args(ref)
    blk = TR.ConvBN(grp, a[0], a[1], a[2], 1, a[3], a[4], EPS, MOM, act=False)
    grp.build()
    out = blk.forward(x.cuda())
    dx = blk.backward(da.cuda())
    got = {"out": _nchw(out), "dx": _nchw(dx), **_block_results("", blk)}
    plain, rounded = DR._run([ref], [""], x, da, False), DR._run([ref], [""], x, da, True)
    d = {n: DR.rel_dist(got[n].cpu(), plain[n]) for n in plain}
    e = {n: DR.rel_dist(rounded[n], plain[n]) for n in plain}
    print("ConvBN act 0: " + ", ".join(f"{n} {d[n]:.2e} (e {e[n]:.2e})" for n in plain))
    assert all(d[n] <= 2 * e[n] for n in plain), (d, e)
    wf, bf = blk.fold()
    f = blk.gamma / torch.sqrt(blk.running_var + EPS)
    assert torch.equal(wf, blk.w * f.view(-1, 1, 1, 1)) and torch.equal(bf, blk.beta - blk.running_mean * f)

    res = []
    for kw in ({}, {"act": True}):
        grp2 = TR.ParamGroups()
        b2 = TR.ConvBN(grp2, a[0], a[1], a[2], 1, a[3], a[4], EPS, MOM, **kw)
        grp2.build()
        o2 = b2.forward(x.cuda())
        d2 = b2.backward(DR._grad_in(torch.Generator().manual_seed(1), B, H, W, c2).cuda())
        res.append((o2, d2, b2.dw.clone(), b2.dgamma.clone(), b2.dbeta.clone(), b2.running_mean.clone(), b2.running_var.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*res)), "ConvBN(act=True) differs from ConvBN without the keyword"
    assert not torch.equal(res[0][0], out)


# ---------------------------------------------------------------------------------------------- train.Attention, train.PSABlock
@pytest.mark.parametrize("kind,B,H,W,C", [("attn", 2, 13, 13, 128), ("attn", 2, 4, 4, 192), ("psa", 2, 13, 13, 128)])
def test_blocks_match_torch_modules_sgd_and_fold(kind, B, H, W, C):
    """train.Attention / train.PSABlock against the nn-module stack in .train(): the output, dx, every parameter gradient and running statistic
    within twice the rounded-against-plain figure; then one SGD step of the three groups against torch.optim.SGD fed the same gradients, and
    fold() against the module stack in .eval(), in checkpoint channel order."""
    _ops()
    import oriented_object_detection_amd.train as TR
    case = AR.block_case(kind, B, H, W, C)
    _, nh, ref, x, dy = case
    tags = AR.ATTN_TAGS if kind == "attn" else AR.PSA_TAGS
    lr, wd = 0.01, 5e-4
    grp = TR.ParamGroups("SGD", lr=lr, momentum=0.9, weight_decay=wd)
    args = [_dev_args(ref[t]) for t in tags]
    blk = TR.Attention(grp, *args, nh, EPS, MOM) if kind == "attn" else TR.PSABlock(grp, *args, nh, EPS, MOM)
    grp.build()
    att = blk if kind == "attn" else blk.attn
    dev = {"qkv": att.qkv, "proj": att.proj, "pe": att.pe, **({} if kind == "attn" else {"ffn0": blk.ffn0, "ffn1": blk.ffn1})}
    inv = att.inv
    assert torch.equal(att.perm.cpu(), AR.qkv_perm(nh))
    out = blk.forward(x.cuda())
    dx = blk.backward(dy.cuda())
    torch.cuda.synchronize()
    got = {"out": _nchw(out), "dx": _nchw(dx)}
    for t in tags:
        got.update(_block_results(t + ".", dev[t], inv if t == "qkv" else None))
    plain, rounded = AR.run_block(case, False), AR.run_block(case, True)
    _assert_within_2e(f"{kind} {B}x{H}x{W}x{C}", got, plain, rounded)

    # fold() in checkpoint order against the module in .eval(), both from the DEVICE's parameters and running statistics
    folded = blk.fold()
    if kind != "attn":  # PSABlock.fold() is keyed by checkpoint-relative names
        folded = {t: folded[BR.PSA_NAMES[t]] for t in tags}
    for t in tags:
        r, d = ref[t], dev[t]
        ck = (lambda v: v[inv]) if t == "qkv" else (lambda v: v)
        with torch.no_grad():
            for dst, src in zip((r.seq[0].weight, r.seq[1].weight, r.seq[1].bias, r.seq[1].running_mean, r.seq[1].running_var),
                                (d.w, d.gamma, d.beta, d.running_mean, d.running_var)):
                dst.copy_(ck(src).double().cpu())
        wf, bf = AR.fold_ref(r)
        assert float((folded[t][0].double().cpu() - wf).abs().max()) <= TS.FOLD_TOL * float(wf.abs().max()), t
        assert float((folded[t][1].double().cpu() - bf).abs().max()) <= TS.FOLD_TOL * max(1.0, float(bf.abs().max())), t

    # one SGD step against torch.optim.SGD fed the device's gradients (device order: the optimiser is element-wise)
    params, grads = [[], [], []], [[], [], []]
    for t in tags:
        for k, (p, gr) in enumerate(((dev[t].w, dev[t].dw), (dev[t].gamma, dev[t].dgamma), (dev[t].beta, dev[t].dbeta))):
            params[k].append(torch.nn.Parameter(p.detach().cpu().clone()))
            grads[k].append(gr.cpu().clone())
    topt = torch.optim.SGD([{"params": params[k], "weight_decay": wd if k == 0 else 0.0} for k in range(3)], lr=lr, momentum=0.9, nesterov=True,
                           foreach=False)
    for k in range(3):
        for p, gr in zip(params[k], grads[k]):
            p.grad = gr
    topt.step()
    grp.step()
    i = [0, 0, 0]
    for t in tags:
        for k, dvp in enumerate((dev[t].w, dev[t].gamma, dev[t].beta)):
            p = params[k][i[k]].detach()
            i[k] += 1
            assert float((dvp.cpu() - p).abs().max()) <= TS.PARAM_TOL * max(1.0, float(p.abs().max())), (t, k)
