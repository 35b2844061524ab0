"""f1, gradient routing through what is not a conv (csrc/routegrad.hip): SPPF's three chained 5x5 max pools, Upsample(2x) + Concat of the FPN, the
plain Concat of the PAN and the gradient sum of a tensor with two consumers -- per element against the fp64 references of tests/route_ref.py
(pinned to torch.autograd by test_train_route_cpu.py); then `train.SPPF` and one assembled multi-branch slice with a fan-out against nn modules
in .train() at the device's bf16 rounding points."""
import pytest
import torch
import torch.nn.functional as F

import route_ref as RR
from bounds import Guarded, U, _check

pytestmark = pytest.mark.gpu

EPS, MOM = RR.EPS, RR.MOM  # Ultralytics' initialize_weights values
BF = 2.0 ** -8             # one bf16 rounding, relative


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


def _ops():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------- SPPF pools
# (B, H, W, C): n-scale, s-scale, the 128-px tile, H != W both ways, C / 8 not a power of two, tiny maps, the map limit, more channel chunks
# than one workgroup's share with a remainder (33 chunks); H * W = 512 and 527 sit on either side of the share rule (2 chunks per workgroup
# while H * W <= 512, 1 above)
POOL_SHAPES = [(2, 13, 13, 128), (2, 13, 13, 256), (3, 4, 4, 64), (2, 13, 9, 64), (2, 9, 13, 64), (1, 3, 7, 24), (2, 2, 1, 8), (1, 1, 1, 8), (1, 32, 32, 8),
               (5, 6, 6, 264), (1, 16, 32, 24), (1, 17, 31, 24)]


def _pool_inputs(B, H, W, C, g):
    few = torch.tensor([-1.0, -0.125, 0.5, 2.0])[torch.randint(0, 4, (B, H, W, C), generator=g)]
    return {"silu": F.silu(torch.randn(B, H, W, C, generator=g) * 2).to(torch.bfloat16),
            "negative": (-(torch.rand(B, H, W, C, generator=g) + 0.1)).to(torch.bfloat16),  # a zero padding would win here
            "constant": torch.full((B, H, W, C), 0.375, dtype=torch.bfloat16),               # every window ties
            "few": few.to(torch.bfloat16)}                                                   # 4 distinct values


def _torch_pools(x):
    """F.max_pool2d chain on the same bf16 values (exact in fp32) -> cat bf16 NHWC."""
    ys = [x.float().permute(0, 3, 1, 2)]
    for _ in range(3):
        ys.append(F.max_pool2d(ys[-1], 5, 1, 2))
    return torch.cat(ys, dim=1).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


@pytest.mark.parametrize("B,H,W,C", POOL_SHAPES)
def test_sppf_pools_forward_and_backward(B, H, W, C):
    """Forward bit-equal to F.max_pool2d; backward within one bf16 rounding of the result plus the fp32 summation error (at most 3 levels x 26
    additions, each 2^-24 relative on the magnitudes summed: 80 x 2^-24 x S, S = the reference run on |dcat|); deterministic; guards intact."""
    ops = _ops()
    O = torch.ops.obbhip
    g = torch.Generator().manual_seed(B * 1000 + H * 37 + W * 5 + C)
    for name, x in _pool_inputs(B, H, W, C, g).items():
        what = f"{B}x{H}x{W}x{C} {name}"
        dcat = torch.randn(B, H, W, 4 * C, generator=g).to(torch.bfloat16)
        cat_ref = _torch_pools(x)
        assert torch.equal(RR.pools_ref(x.double()), cat_ref.double()), what  # the reference's own forward
        ref = RR.pools_bwd_ref(cat_ref.double(), dcat.double())
        S = RR.pools_bwd_ref(cat_ref.double(), dcat.double().abs())

        xd, dd = x.cuda(), dcat.cuda()
        gc = Guarded((B, H, W, 4 * C), torch.bfloat16)
        O.sppf_pools_fwd(xd, gc.out)
        cat = gc.get(what + " cat")
        assert torch.equal(cat.cpu(), cat_ref), what + ": cat is not bit-equal to F.max_pool2d"
        gx = Guarded((B, H, W, C), torch.bfloat16)
        O.sppf_pools_bwd(cat, dd, gx.out)
        dx = gx.get(what + " dx")
        _check(what + " dx", dx, ref, BF * ref.abs() + 80 * U * S)
        assert torch.equal(ops.sppf_pools_fwd_bf16(xd), cat) and torch.equal(ops.sppf_pools_bwd_bf16(cat, dd), dx), what + ": second call differs"


def test_sppf_pools_argument_checks():
    ops = _ops()
    from oriented_object_detection_amd import _lib
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.ObbHipError, match="map"):
        ops.sppf_pools_fwd_bf16(z(1, 33, 8, 8))
    with pytest.raises(_lib.ObbHipError, match="map"):
        ops.sppf_pools_bwd_bf16(z(1, 8, 33, 32), z(1, 8, 33, 32))
    with pytest.raises(_lib.ObbHipError, match="multiple of 8"):
        ops.sppf_pools_fwd_bf16(z(1, 4, 4, 12))
    with pytest.raises(_lib.ObbHipError, match="multiple of 8"):
        ops.sppf_pools_bwd_bf16(z(1, 4, 4, 48), z(1, 4, 4, 48))
    with pytest.raises(_lib.ObbHipError, match="NULL"):
        ops._call("obb_sppf_pools_fwd_bf16", ops.ctx(), ops._p(z(1, 4, 4, 8)), 1, 4, 4, 8, ops._p(None), ops._stream())
    with pytest.raises(_lib.ObbHipError, match="at least 1"):
        ops._call("obb_sppf_pools_fwd_bf16", ops.ctx(), ops._p(z(1, 4, 4, 8)), 0, 4, 4, 8, ops._p(z(1, 4, 4, 32)), ops._stream())


# ---------------------------------------------------------------------------------------------- upsample + concat
# (B, H, W, Ca, Cb, up): n FPN (x2), s FPN, PAN (x2), non-square, tiny (x2)
UPCAT_SHAPES = [(2, 13, 13, 256, 128, 2), (2, 26, 26, 128, 128, 2), (2, 13, 13, 512, 256, 2), (2, 26, 26, 64, 128, 1), (2, 13, 13, 128, 256, 1),
                (2, 9, 13, 24, 40, 2), (1, 1, 1, 8, 8, 2), (1, 1, 1, 8, 8, 1)]


@pytest.mark.parametrize("B,H,W,Ca,Cb,up", UPCAT_SHAPES)
def test_upcat_forward_and_backward(B, H, W, Ca, Cb, up):
    """Forward bit-equal to cat(upsample(a), b); backward within one bf16 rounding of the result + 5 x 2^-24 x the sum of the magnitudes of the
    terms (at most up^2 + 1 = 5 fp32 additions); db bit-equal when not accumulating; with accumulation the reference adds the prior bf16 buffer
    in fp64; a NULL half is skipped and writes nothing."""
    ops = _ops()
    O = torch.ops.obbhip
    g = torch.Generator().manual_seed(B * 1000 + H * 37 + W * 5 + Ca + Cb + up)
    what = f"{B}x{H}x{W} {Ca}+{Cb} up{up}"
    a = torch.randn(B, H, W, Ca, generator=g).to(torch.bfloat16)
    b = torch.randn(B, H * up, W * up, Cb, generator=g).to(torch.bfloat16)
    dout = torch.randn(B, H * up, W * up, Ca + Cb, generator=g).to(torch.bfloat16)
    da0 = torch.randn(B, H, W, Ca, generator=g).to(torch.bfloat16)
    db0 = torch.randn(B, H * up, W * up, Cb, generator=g).to(torch.bfloat16)
    ad, bd, dd = a.cuda(), b.cuda(), dout.cuda()

    go = Guarded((B, H * up, W * up, Ca + Cb), torch.bfloat16)
    O.upcat_fwd(ad, bd, up, go.out)
    out = go.get(what + " out")
    assert torch.equal(out.cpu().double(), RR.upcat_ref(a.double(), b.double(), up)), what + ": forward is not a bit-exact copy"
    assert torch.equal(ops.upcat_fwd_bf16(ad, bd, up), out)

    # overwrite
    ra, rb = RR.upcat_bwd_ref(dout.double(), Ca, up)
    sa, _ = RR.upcat_bwd_ref(dout.double().abs(), Ca, up)
    ga, gb = Guarded((B, H, W, Ca), torch.bfloat16), Guarded((B, H * up, W * up, Cb), torch.bfloat16)
    O.upcat_bwd(dd, H, W, Ca, up, ga.out, gb.out, False, False)
    da, db = ga.get(what + " da"), gb.get(what + " db")
    _check(what + " da", da, ra, BF * ra.abs() + 5 * U * sa)
    assert torch.equal(db.cpu().double(), rb), what + ": db is not a bit-exact copy"
    da2, db2 = ops.upcat_bwd_bf16(dd, Ca, up)
    assert torch.equal(da2, da) and torch.equal(db2, db), what + ": second call differs"

    # accumulate: the prior bf16 buffer is one more term
    ra, rb = RR.upcat_bwd_ref(dout.double(), Ca, up, da0.double(), db0.double())
    sa, sb = RR.upcat_bwd_ref(dout.double().abs(), Ca, up, da0.double().abs(), db0.double().abs())
    ga, gb = Guarded((B, H, W, Ca), torch.bfloat16, da0), Guarded((B, H * up, W * up, Cb), torch.bfloat16, db0)
    O.upcat_bwd(dd, H, W, Ca, up, ga.out, gb.out, True, True)
    _check(what + " da accum", ga.get(what + " da accum"), ra, BF * ra.abs() + 5 * U * sa)
    _check(what + " db accum", gb.get(what + " db accum"), rb, BF * rb.abs() + 5 * U * sb)
    pa, pb = ops.upcat_bwd_bf16(dd, Ca, up, da=da0.cuda(), db=db0.cuda())  # the wrapper: a given buffer is accumulated into
    assert torch.equal(pa, ga.out) and torch.equal(pb, gb.out)

    # NULL halves: the other half is written alone, and a buffer that was not handed over keeps every byte
    ga, gb = Guarded((B, H, W, Ca), torch.bfloat16), Guarded((B, H * up, W * up, Cb), torch.bfloat16)
    O.upcat_bwd(dd, H, W, Ca, up, ga.out, None, False, False)
    assert torch.equal(ga.get(what + " da alone"), da)
    torch.cuda.synchronize()
    assert bool((gb.raw == 0xFF).all()), what + ": db written although NULL"
    ga = Guarded((B, H, W, Ca), torch.bfloat16)
    O.upcat_bwd(dd, H, W, Ca, up, None, gb.out, False, False)
    assert torch.equal(gb.get(what + " db alone"), db)
    assert bool((ga.raw == 0xFF).all()), what + ": da written although NULL"
    only_a, none_b = ops.upcat_bwd_bf16(dd, Ca, up, need_db=False)
    assert none_b is None and torch.equal(only_a, da)


def test_upcat_argument_checks():
    ops = _ops()
    from oriented_object_detection_amd import _lib
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.ObbHipError, match="Ca = 12"):
        ops.upcat_fwd_bf16(z(1, 4, 4, 12), z(1, 4, 4, 8), 1)
    with pytest.raises(_lib.ObbHipError, match="Cb = 12"):
        ops.upcat_fwd_bf16(z(1, 4, 4, 8), z(1, 8, 8, 12), 2)
    with pytest.raises(_lib.ObbHipError, match="Ca = 12"):
        ops.upcat_bwd_bf16(z(1, 4, 4, 20), 12, 1)
    with pytest.raises(_lib.ObbHipError, match="up = 3"):
        ops.upcat_fwd_bf16(z(1, 2, 2, 8), z(1, 6, 6, 8), 3)
    with pytest.raises(_lib.ObbHipError, match="up = 3"):
        ops.upcat_bwd_bf16(z(1, 6, 6, 16), 8, 3)
    with pytest.raises(_lib.ObbHipError, match="NULL"):
        ops._call("obb_upcat_fwd_bf16", ops.ctx(), ops._p(z(1, 2, 2, 8)), ops._p(None), 1, 2, 2, 8, 8, 1, ops._p(z(1, 2, 2, 16)), ops._stream())
    with pytest.raises(_lib.ObbHipError, match="NULL"):
        ops._call("obb_upcat_bwd_bf16", ops.ctx(), ops._p(None), 1, 2, 2, 8, 8, 1, ops._p(z(1, 2, 2, 8)), ops._p(z(1, 2, 2, 8)), 0, 0, ops._stream())


# ---------------------------------------------------------------------------------------------- train.SPPF, and a slice with a fan-out
def _rel(d, r):
    return float((d.float().cpu() - r.detach()).abs().max()) / float(r.detach().abs().max())


def _block_errors(tag, blk, ref):
    return {f"{tag}.dW": _rel(blk.dw, ref.w.grad), f"{tag}.dgamma": _rel(blk.dgamma, ref.bn.weight.grad), f"{tag}.dbeta": _rel(blk.dbeta, ref.bn.bias.grad),
            f"{tag}.rmean": _rel(blk.running_mean, ref.bn.running_mean), f"{tag}.rvar": _rel(blk.running_var, ref.bn.running_var)}


FLOOR = RR.FLOOR  # (with SPPF_MEASURED in route_ref.py: the step tests read the same bounds)


def _assert_measured(e, measured):
    """e: name -> max |d| / max |ref| ("out", "dx", "cv1.dW", ...), every one asserted at 2.5 x ITS OWN measured figure (MI355X)."""
    assert set(e) == set(measured), set(e) ^ set(measured)
    for n, v in e.items():
        bound = max(2.5 * measured[n], FLOOR[n.split(".")[-1]])
        assert v <= bound, (n, v, bound, e)


# measured (MI355X), max |d| / max |ref| of every compared quantity
SPPF_MEASURED = RR.SPPF_MEASURED
SLICE_MEASURED = {"out": 6.17e-3, "dx": 7.52e-3, "dskip": 4.74e-3,
                  "cv1.dW": 4.81e-3, "cv1.dgamma": 1.17e-2, "cv1.dbeta": 1.36e-2, "cv1.rmean": 3.28e-8, "cv1.rvar": 3.90e-8,
                  "cv2.dW": 8.65e-3, "cv2.dgamma": 1.89e-3, "cv2.dbeta": 5.56e-3, "cv2.rmean": 4.44e-6, "cv2.rvar": 1.86e-6,
                  "fpn.dW": 3.41e-3, "fpn.dgamma": 5.01e-3, "fpn.dbeta": 5.44e-3, "fpn.rmean": 2.59e-6, "fpn.rvar": 1.59e-6,
                  "down.dW": 4.43e-3, "down.dgamma": 2.43e-3, "down.dbeta": 3.74e-3, "down.rmean": 1.62e-5, "down.rvar": 6.45e-6,
                  "pan.dW": 2.33e-3, "pan.dgamma": 2.67e-3, "pan.dbeta": 1.17e-3, "pan.rmean": 2.93e-5, "pan.rvar": 1.31e-5}


@pytest.mark.parametrize("B,H,W,c1,c2", [(2, 13, 13, 256, 256), (2, 4, 4, 128, 128)])
def test_sppf_block_matches_torch_modules(B, H, W, c1, c2):
    """train.SPPF against Conv/BN/SiLU x 2 around F.max_pool2d in .train(): output, dx, both dW, dgamma, dbeta and the running statistics."""
    _ops()
    import oriented_object_detection_amd.train as TR
    cv1, cv2, x, da = RR.sppf_case(B, H, W, c1, c2)

    grp = TR.ParamGroups("SGD", lr=0.01, momentum=0.9, weight_decay=5e-4)
    blk = TR.SPPF(grp, cv1.device_args(), cv2.device_args(), eps=EPS, momentum=MOM)
    grp.build()
    out = blk.forward(x.cuda())
    dx = blk.backward(da.cuda())
    torch.cuda.synchronize()

    xr = _nchw(x).requires_grad_(True)
    a1_ref, out_ref = RR.ref_sppf(cv1, cv2, xr, _nchw(blk.cat[..., :c1 // 2]))
    out_ref.backward(_nchw(da))
    e_a1 = _rel(_nchw(blk.cat[..., :c1 // 2]), a1_ref)
    e = {"out": _rel(_nchw(out), out_ref), "dx": _rel(_nchw(dx), xr.grad), **_block_errors("cv1", blk.cv1, cv1), **_block_errors("cv2", blk.cv2, cv2)}
    print(f"SPPF {B}x{H}x{W} {c1}->{c2}: a1 {e_a1:.2e}, " + ", ".join(f"{n} {v:.2e}" for n, v in e.items()))
    assert e_a1 <= 1.2e-2, e_a1  # the existing ConvBN bound; measured (MI355X): 3.24e-4 / 0
    # cv1's dgamma / dbeta are the large figures (1.54e-2 is past the 1.5e-2 of the loosest existing chain), and not by a fault of the kernels:
    # the device stores cv2's dz, dcat and the pools' dx in bf16, autograd rounds no gradient, and the pools pile those roundings onto the few
    # window maxima of a channel, whose signed sum dbeta is.  test_train_route_cpu.py::test_bf16_gradients_explain_cv1_dbeta reproduces the
    # figures on the CPU from the reference alone: rounding exactly these gradients moves cv1 dbeta by 1.54e-2, dgamma by 1.09e-2, cv2 dW by
    # 4.84e-3 and cv2 dgamma / dbeta by nothing.
    _assert_measured(e, SPPF_MEASURED[(B, H, W, c1, c2)])


def test_fanout_slice_matches_autograd_and_sgd():
    """x -> SPPF -> y;  UpCat(2)(y, skip) -> ConvBN 1x1 -> t;  t -> ConvBN 3x3 s2 -> d;  UpCat(1)(d, y) -> ConvBN 1x1 -> out.  y feeds two
    consumers: its gradient is the PAN concat's half, then the FPN upsample's half accumulated into the same buffer.  out, dx, dskip and every
    parameter gradient against autograd at the same forward rounding points (pool input pinned as above); then one SGD step of the three groups
    against torch.optim.SGD fed the same gradients."""
    _ops()
    import oriented_object_detection_amd.train as TR
    B, H, W, c = 2, 13, 13, 128
    g = torch.Generator().manual_seed(20251)
    ref = {"cv1": RR.RefConvBN(g, c, c // 2), "cv2": RR.RefConvBN(g, 2 * c, c), "fpn": RR.RefConvBN(g, 2 * c, c), "down": RR.RefConvBN(g, c, c, 3, 2),
           "pan": RR.RefConvBN(g, 2 * c, c)}
    x = torch.randn(B, H, W, c, generator=g).to(torch.bfloat16)
    skip = torch.randn(B, 2 * H, 2 * W, c, generator=g).to(torch.bfloat16)
    dout = (torch.randn(B, H, W, c, generator=g) * 0.1).to(torch.bfloat16)

    lr, wd = 0.01, 5e-4
    grp = TR.ParamGroups("SGD", lr=lr, momentum=0.9, weight_decay=wd)
    sppf = TR.SPPF(grp, ref["cv1"].device_args(), ref["cv2"].device_args(), eps=EPS, momentum=MOM)
    mk = lambda r: TR.ConvBN(grp, *r.device_args()[:3], r.s, *r.device_args()[3:], EPS, MOM)
    fpn, down, pan = mk(ref["fpn"]), mk(ref["down"]), mk(ref["pan"])
    up2, cat1 = TR.UpCat(2), TR.UpCat(1)
    grp.build()
    y = sppf.forward(x.cuda())
    t = fpn.forward(up2.forward(y, skip.cuda()))
    d = down.forward(t)
    out = pan.forward(cat1.forward(d, y))
    dd, dy = cat1.backward(pan.backward(dout.cuda()))          # y's first gradient (a fresh buffer)
    dy_first = dy.clone()
    dy2, dskip = up2.backward(fpn.backward(down.backward(dd)), da=dy)  # ... and its second, accumulated into the same buffer
    assert dy2.data_ptr() == dy.data_ptr() and not torch.equal(dy, dy_first)
    dx = sppf.backward(dy)
    torch.cuda.synchronize()

    xr, sr = _nchw(x).requires_grad_(True), _nchw(skip).requires_grad_(True)
    a1_ref, y_ref = RR.ref_sppf(ref["cv1"], ref["cv2"], xr, _nchw(sppf.cat[..., :c // 2]))
    t_ref = ref["fpn"](torch.cat([F.interpolate(y_ref, scale_factor=2, mode="nearest"), sr], dim=1))
    out_ref = ref["pan"](torch.cat([ref["down"](t_ref), y_ref], dim=1))
    out_ref.backward(_nchw(dout))
    e_a1 = _rel(_nchw(sppf.cat[..., :c // 2]), a1_ref)
    blocks = {"cv1": sppf.cv1, "cv2": sppf.cv2, "fpn": fpn, "down": down, "pan": pan}
    e = {"out": _rel(_nchw(out), out_ref), "dx": _rel(_nchw(dx), xr.grad), "dskip": _rel(_nchw(dskip), sr.grad)}
    for n, blk in blocks.items():
        e.update(_block_errors(n, blk, ref[n]))
    print(f"slice: a1 {e_a1:.2e}, " + ", ".join(f"{n} {v:.2e}" for n, v in e.items()))
    assert e_a1 <= 1.2e-2, e_a1  # the existing ConvBN bound; measured (MI355X): 0 (bit-equal)
    # cv1 dgamma / dbeta: bf16 gradients piled up by the pools (see test_sppf_block_matches_torch_modules); the running statistics grow down the
    # chain (pan, the last block, has every earlier flipped bf16 rounding in its input)
    _assert_measured(e, SLICE_MEASURED)

    # one SGD step of the three groups (weights decay, norm weights and biases do not) against torch.optim.SGD on the same gradients
    names = list(blocks)
    topt = torch.optim.SGD([{"params": [ref[n].w for n in names], "weight_decay": wd}, {"params": [ref[n].bn.weight for n in names], "weight_decay": 0.0},
                            {"params": [ref[n].bn.bias for n in names], "weight_decay": 0.0}], lr=lr, momentum=0.9, nesterov=True, foreach=False)
    for n in names:
        for p, gr in zip(ref[n].params(), (blocks[n].dw, blocks[n].dgamma, blocks[n].dbeta)):
            p.grad = gr.cpu().clone()
    topt.step()
    grp.step()
    for n in names:
        for p, dv in zip(ref[n].params(), (blocks[n].w, blocks[n].gamma, blocks[n].beta)):
            assert float((dv.cpu() - p.detach()).abs().max()) <= 2e-6 * max(1.0, float(p.detach().abs().max())), n
