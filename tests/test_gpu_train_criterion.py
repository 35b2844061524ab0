"""The fused OBB training criterion (csrc/criterion.hip: obb_crit_decode, obb_crit_loss; train.OBBCriterion, train.DetectHead) per element against
the fp64 restatement and bounds of criterion_ref.py.  Outputs go into Guarded buffers (NaN-filled, between guard bands); every check prints its
worst |err| / bound.  Shapes: imgsz 128 x 128 (levels 16^2, 8^2, 4^2, A = 336) and 96 x 160 (12 x 20, 6 x 10, 3 x 5), B in {1, 2}, nc in {1, 12,
15}, box logits in bf16 and fp32."""
import math

import numpy as np
import pytest
import torch

import criterion_ref as CR
from bounds import U, Guarded, _check
from oracle import loss as ol

pytestmark = pytest.mark.gpu

SHAPES = [((128, 128), 2, 12, "bf16"), ((96, 160), 2, 15, "fp32"), ((96, 160), 1, 1, "bf16"), ((128, 128), 1, 15, "fp32")]
_ids = lambda c: f"{c[0][0]}x{c[0][1]}-B{c[1]}-nc{c[2]}-{c[3]}"


def _ops():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    return ops, _lib


def _dev_head(box, cls, ang, dtype):
    bd = torch.bfloat16 if dtype == "bf16" else torch.float32
    return [b.to(bd).cuda() for b in box], [c.cuda() for c in cls], [a.cuda() for a in ang]


def _flat(box, cls, ang):
    return CR.cat_levels(box), CR.cat_levels(cls), CR.cat_levels(ang)[..., 0]


class _Outs:
    """Guarded gradient buffers of one crit_loss call"""

    def __init__(self, box, cls, ang):
        self.b = [Guarded(tuple(t.shape), torch.bfloat16) for t in box]
        self.c = [Guarded(tuple(t.shape), torch.float32) for t in cls]
        self.a = [Guarded(tuple(t.shape), torch.float32) for t in ang]

    def out(self):
        return [g.out for g in self.b], [g.out for g in self.c], [g.out for g in self.a]

    def get(self, what):
        f = lambda gs, n: CR.cat_levels([g.get(f"{what} {n}[{i}]").float().cpu() for i, g in enumerate(gs)])
        return f(self.b, "d_box"), f(self.c, "d_cls"), f(self.a, "d_angle")[..., 0]

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((g.raw == 0xFF).all()) for g in self.b + self.c + self.a)


def _check_loss(what, got_items, got_tss, gb, gc, ga, ref, bound):
    _check(f"{what} items", got_items, ref["items"], bound["items"])
    _check(f"{what} tss", got_tss, ref["tss"], bound["tss"])
    _check(f"{what} d_box", gb, ref["d_box"], bound["d_box"])
    _check(f"{what} d_cls", gc, ref["d_cls"], bound["d_cls"])
    _check(f"{what} d_angle", ga, ref["d_ang"], bound["d_ang"])


# ---------------------------------------------------------------------------------------------- 1. decode
@pytest.mark.parametrize("case", SHAPES, ids=_ids)
def test_decode(case):
    ops, _ = _ops()
    imgsz, B, nc, dtype = case
    box, cls, ang = CR.make_head(20, imgsz, B, nc, dtype)
    dbox, dcls, dang = _dev_head(box, cls, ang, dtype)
    A = sum(h * w for h, w in CR.level_shapes(imgsz))
    ps, pb, ap, st = Guarded((B, A, nc), torch.float32), Guarded((B, A, 5), torch.float32), Guarded((A, 2), torch.float32), Guarded((A,), torch.float32)
    torch.ops.obbhip.crit_decode(*dbox, *dcls, *dang, ps.out, pb.out, ap.out, st.out)
    (rps, rpb), (bps, bpb) = CR.decode_bounds(*_flat(box, cls, ang), imgsz)
    _check("pd_scores", ps.get("pd_scores"), rps, bps)
    _check("pd_bboxes", pb.get("pd_bboxes"), rpb, bpb)
    anc, strides = CR.anchors(imgsz)
    assert torch.equal(ap.get("anc_points").double().cpu(), anc * strides[:, None]) and torch.equal(st.get("stride").double().cpu(), strides)
    again = ops.crit_decode(dbox, dcls, dang)
    assert torch.equal(again[0], ps.out) and torch.equal(again[1], pb.out) and torch.equal(again[2], ap.out) and torch.equal(again[3], st.out)


# ---------------------------------------------------------------------------------------------- 2. + 3. loss given an assignment, structure
@pytest.mark.parametrize("case", SHAPES, ids=_ids)
def test_loss_given_assignment(case):
    ops, _ = _ops()
    imgsz, B, nc, dtype = case
    box, cls, ang = CR.make_head(30, imgsz, B, nc, dtype)
    tb, ts, fg = CR.hand_targets(30, imgsz, B, nc, small_tss=(nc == 1))
    fb, fc, fa = _flat(box, cls, ang)
    ref, bound = CR.crit_bounds(fb, fc, fa, tb, ts, fg, imgsz)
    if nc == 1:
        assert float(ts.sum()) < 1 and float(ref["tss"]) == 1.0  # the case with sum target_scores < 1
    ltrb = CR.target_ltrb(ref["tgt"], CR.anchors(imgsz)[0][fg.nonzero(as_tuple=True)[1]], "no_clamp")
    assert float(ltrb.min()) == 0 and float(ltrb.max()) > 15  # both ends of the clamp are hit
    dbox, dcls, dang = _dev_head(box, cls, ang, dtype)
    o = _Outs(dbox, dcls, dang)
    items, tss, *_ = ops.crit_loss(dbox, dcls, dang, tb.cuda(), ts.cuda(), fg.cuda(), out=o.out())
    gb, gc, ga = o.get("crit_loss")
    assert bool(torch.isfinite(items).all())
    _check_loss("given assignment", items, tss, gb, gc, ga, ref, bound)
    assert bool((gb[~fg] == 0).all()) and bool((ga[~fg] == 0).all())  # background anchors: exact zeros
    o2 = _Outs(dbox, dcls, dang)
    items2, tss2, *_ = ops.crit_loss(dbox, dcls, dang, tb.cuda(), ts.cuda(), fg.cuda(), out=o2.out())
    gb2, gc2, ga2 = o2.get("crit_loss again")
    assert torch.equal(items, items2) and torch.equal(tss, tss2) and torch.equal(gb, gb2) and torch.equal(gc, gc2) and torch.equal(ga, ga2)


def test_no_foreground():
    ops, _ = _ops()
    imgsz, B, nc = (96, 160), 2, 12
    box, cls, ang = CR.make_head(40, imgsz, B, nc, "bf16")
    dbox, dcls, dang = _dev_head(box, cls, ang, "bf16")
    A = sum(h * w for h, w in CR.level_shapes(imgsz))
    tb, ts, fg = torch.zeros((B, A, 5)), torch.zeros((B, A, nc)), torch.zeros((B, A), dtype=torch.bool)
    o = _Outs(dbox, dcls, dang)
    items, tss, *_ = ops.crit_loss(dbox, dcls, dang, tb.cuda(), ts.cuda(), fg.cuda(), out=o.out())
    gb, gc, ga = o.get("no foreground")
    assert float(items[0]) == 0 and float(items[2]) == 0 and float(tss) == 1.0
    assert bool((gb == 0).all()) and bool((ga == 0).all())
    fb, fc, fa = _flat(box, cls, ang)
    ref, bound = CR.crit_bounds(fb, fc, fa, tb, ts, fg, imgsz)
    want = B * CR.GAINS[1] * torch.sigmoid(fc.double())
    assert float((want - ref["d_cls"]).abs().max()) <= 1e-12
    _check("no foreground d_cls = B g_cls sigmoid(x)", gc, want, bound["d_cls"])
    _check("no foreground L_cls", items[1:2], ref["items"][1:2], bound["items"][1:2])


def test_fp32_and_bf16_logits_agree_bit_for_bit():
    ops, _ = _ops()
    imgsz, B, nc = (96, 160), 2, 15
    box, cls, ang = CR.make_head(50, imgsz, B, nc, "bf16")  # bf16 values held in fp32
    tb, ts, fg = CR.hand_targets(50, imgsz, B, nc)
    res = []
    for dtype in ("bf16", "fp32"):
        dbox, dcls, dang = _dev_head(box, cls, ang, dtype)
        dec = ops.crit_decode(dbox, dcls, dang)
        items, tss, gb, gc, ga = ops.crit_loss(dbox, dcls, dang, tb.cuda(), ts.cuda(), fg.cuda())
        res.append(list(dec) + [items, tss] + gb + gc + ga)
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_refusals_leave_outputs_untouched():
    ops, lib = _ops()
    imgsz, B, nc = (128, 128), 1, 12
    box, cls, ang = CR.make_head(60, imgsz, B, nc, "bf16")
    dbox, dcls, dang = _dev_head(box, cls, ang, "bf16")
    tb, ts, fg = (t.cuda() for t in CR.hand_targets(60, imgsz, B, nc))
    o = _Outs(dbox, dcls, dang)
    with pytest.raises(ValueError):
        ops.crit_loss(dbox[:2], dcls[:2], dang[:2], tb, ts, fg, out=o.out())
    with pytest.raises(ValueError):
        ops.crit_loss(dbox, dcls, dang, tb[:, :-1].contiguous(), ts, fg, out=o.out())
    with pytest.raises(ValueError):
        ops.crit_loss(dbox, [c[..., :0].contiguous() for c in dcls], dang, tb, ts, fg, out=o.out())
    with pytest.raises(ValueError):
        ops.crit_decode(dbox, dcls, [a[:, :-1].contiguous() for a in dang])
    # the library's own checks (past the Python layer): nc = 65, and a zero-height level
    A = tb.shape[1]
    wide = [torch.zeros((*c.shape[:3], 65), device="cuda") for c in dcls]
    items, tss = Guarded((3,), torch.float32), Guarded((1,), torch.float32)
    ob, oc, oa = o.out()
    with pytest.raises(lib.ObbHipError):
        torch.ops.obbhip.crit_loss(*dbox, *wide, *dang, tb, torch.zeros((B, A, 65), device="cuda"), fg.view(torch.uint8), 7.5, 0.5, 1.5, *ob, *oc, *oa,
                                   items.out, tss.out)
    ps, pb, ap, st = Guarded((B, A, nc), torch.float32), Guarded((B, A, 5), torch.float32), Guarded((A, 2), torch.float32), Guarded((A,), torch.float32)
    flat0 = [dbox[0][:, :0].contiguous()] + dbox[1:]
    with pytest.raises(lib.ObbHipError):
        torch.ops.obbhip.crit_decode(*flat0, *dcls, *dang, ps.out, pb.out, ap.out, st.out)
    assert o.untouched()
    for g in (items, tss, ps, pb, ap, st):
        assert bool((g.raw == 0xFF).all())


# ---------------------------------------------------------------------------------------------- 4. agreement with the existing kernels
def test_terms_agree_with_the_standalone_loss_kernels():
    """On the gathered foreground pairs L_box, L_dfl and L_cls equal ops.probiou_loss / dfl_loss / bce_loss fed the device's own decode and tss, to
    within the sum-order floor (additions + 8) u sum |elements| (all elements >= 0: sum |elements| = the term)."""
    ops, _ = _ops()
    imgsz, B, nc = (128, 128), 2, 12
    box, cls, ang = CR.make_head(70, imgsz, B, nc, "fp32")
    tb, ts, fg = CR.hand_targets(70, imgsz, B, nc)
    dbox, dcls, dang = _dev_head(box, cls, ang, "fp32")
    items, tss, *_ = ops.crit_loss(dbox, dcls, dang, tb.cuda(), ts.cuda(), fg.cuda(), gains=(1.0, 1.0, 1.0))
    _, pb, _, st = ops.crit_decode(dbox, dcls, dang)
    tssf = float(tss)
    bi, ai = fg.cuda().nonzero(as_tuple=True)
    s = st[ai][:, None]
    pred = torch.cat([pb[bi, ai, :4] / s, pb[bi, ai, 4:]], 1).contiguous()   # (powers of two: the grid-unit values the loss kernel decodes)
    tgt = torch.cat([tb.cuda()[bi, ai, :4] / s, tb.cuda()[bi, ai, 4:]], 1).contiguous()
    w = ts.cuda().sum(-1)[bi, ai].contiguous()
    anc = CR.anchors(imgsz, torch.float32)[0].cuda()[ai]
    ltrb = torch.stack([anc[:, 0] - (tgt[:, 0] - tgt[:, 2] * 0.5), anc[:, 1] - (tgt[:, 1] - tgt[:, 3] * 0.5), (tgt[:, 0] + tgt[:, 2] * 0.5) - anc[:, 0],
                        (tgt[:, 1] + tgt[:, 3] * 0.5) - anc[:, 1]], 1).contiguous()
    fbox = CR.cat_levels(dbox)
    l_box, _ = ops.probiou_loss(pred, tgt, w, tssf)
    l_dfl, _ = ops.dfl_loss(fbox[bi, ai].contiguous(), ltrb, w, tssf)
    l_cls, _ = ops.bce_loss(CR.cat_levels(dcls).contiguous(), ts.cuda(), tssf)
    n = B * fg.shape[1]
    for k, (name, other, adds) in enumerate((("L_box", l_box, CR.depth(n)), ("L_cls", l_cls, CR.depth(n * nc) + CR.depth(n, nc)), ("L_dfl", l_dfl, CR.depth(n, 16)))):
        d, floor = abs(float(items[k]) - float(other)), (adds + 8) * U * abs(float(other))
        print(f"  {name}: fused {float(items[k])!r} standalone {float(other)!r} |d| / floor = {d / floor:.3f}")
        assert d <= floor


def test_probiou_gradient_is_bit_equal_through_unit_chains():
    """Probes whose chain to a logit is a known exact factor.  The l and r logits all equal (l = r = 7.5), the t and b logits one-hot at bin 3 (t = b
    = 3 exactly: exp(-200) = 0), so xf = yf = 0 and the box is 15 x 6; a = 0 (sigma = 1 / 2, theta = pi / 4): d_angle = g_theta * fl(pi / 4) (one rounding), and with the target centred on the prediction (g_x = g_y = 0), the l side's last
    bin: d_box[15] = bf16((1 / 16) (15 - 7.5) g_w), DFL gain 0.  g from ops.probiou_loss on the same pairs."""
    ops, _ = _ops()
    imgsz, B, nc = (128, 128), 1, 1
    shapes = CR.level_shapes(imgsz)
    A = sum(h * w for h, w in shapes)
    dbox = [torch.zeros((B, h, w, 64), device="cuda") for h, w in shapes]
    for t in dbox:
        for o in (16, 48):
            t[..., o:o + 16] = -200.0
            t[..., o + 3] = 0.0
    dcls = [torch.zeros((B, h, w, nc), device="cuda") for h, w in shapes]
    dang = [torch.zeros((B, h, w, 1), device="cuda") for h, w in shapes]
    anc, st = CR.anchors(imgsz, torch.float32)
    g = torch.Generator().manual_seed(5)
    r = torch.rand((A, 3), generator=g)
    tb = torch.empty((B, A, 5))
    tb[0, :, 0], tb[0, :, 1] = anc[:, 0] * st, anc[:, 1] * st
    tb[0, :, 2], tb[0, :, 3] = (6 + 12 * r[:, 0]) * st, (6 + 12 * r[:, 1]) * st
    tb[0, :, 4] = (r[:, 2] - 0.25) * math.pi
    ts = torch.full((B, A, nc), 0.5)  # weight 0.5, tss = A / 2: exact
    fg = torch.ones((B, A), dtype=torch.bool)
    items, tss, gb, gc, ga = ops.crit_loss(dbox, dcls, dang, tb.cuda(), ts.cuda(), fg.cuda(), gains=(1.0, 1.0, 0.0))
    th = float(np.float32(0.25) * np.float32(math.pi))
    pred = torch.tensor([[0.0, 0.0, 15.0, 6.0, th]]).repeat(A, 1)
    pred[:, :2] = anc
    tgt = torch.cat([tb[0, :, :4] / st[:, None], tb[0, :, 4:]], 1)
    _, gp = ops.probiou_loss(pred.cuda(), tgt.cuda().contiguous(), torch.full((A,), 0.5, device="cuda"), float(tss))
    torch.cuda.synchronize()
    assert float(gp[:, 4].abs().max()) > 0 and float(gp[:, 2].abs().max()) > 0
    want_a = gp[:, 4] * torch.tensor(np.float32(math.pi) * np.float32(0.25), device="cuda")
    assert torch.equal(CR.cat_levels(ga)[0, :, 0], want_a)
    want_b = (gp[:, 2] * 0.46875).to(torch.bfloat16)  # p_15 (15 - E) = (1 / 16) 7.5, exact
    assert torch.equal(CR.cat_levels(gb)[0, :, 15], want_b)


# ---------------------------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("case", CR.E2E_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-B{c[1]}-nc{c[2]}-{c[3]}-s{c[4]}")
def test_end_to_end(case):
    _ops()
    from oriented_object_detection_amd import train
    imgsz, B, nc, dtype, seed = case
    box, cls, ang = CR.make_head(seed, imgsz, B, nc, dtype)
    gl, gb, mk = CR.make_gt(seed, imgsz, B, nc)
    fb, fc, fa = _flat(box, cls, ang)
    ps, pb, ap, _ = CR.decode_px(fb.double(), fc.double(), fa.double(), imgsz)
    tl, tbx, tsc, fg, ti, _, _ = ol.rotated_tal_assign(ps, pb, ap, gl.long()[..., None], gb.double(), mk[..., None].double())
    dbox, dcls, dang = _dev_head(box, cls, ang, dtype)
    crit = train.OBBCriterion(nc)
    items, (d_box, d_cls, d_ang) = crit(dbox, dcls, dang, gl.cuda(), gb.cuda(), mk.cuda())
    torch.cuda.synchronize()
    last = crit.last
    # the discrete outputs: identical to the fp64 oracle's, nothing excluded
    assert torch.equal(last["fg_mask"].cpu(), fg) and int(fg.sum()) >= 8
    assert torch.equal(last["target_gt_idx"].cpu().long(), ti) and torch.equal(last["target_labels"].cpu().long(), tl)
    assert torch.equal(last["target_bboxes"].cpu().double(), tbx)
    assert torch.equal(last["target_scores"].cpu() > 0, tsc > 0)
    # then the criterion on the device's own (fp32) target scores: the assigner's accuracy is test_gpu_train_loss.py's subject
    ref, bound = CR.crit_bounds(fb, fc, fa, last["target_bboxes"].cpu(), last["target_scores"].cpu(), fg, imgsz)
    _check_loss("end to end", items, last["tss"], CR.cat_levels([t.float().cpu() for t in d_box]), CR.cat_levels([t.cpu() for t in d_cls]),
                CR.cat_levels([t.cpu() for t in d_ang])[..., 0], ref, bound)
    if case is CR.E2E_CASES[0]:  # one case under a single-stream graph capture + replay: bit-equal to eager
        eager = [items.clone()] + [t.clone() for t in d_box + d_cls + d_ang]
        dgl, dgb, dmk = gl.cuda(), gb.cuda(), mk.cuda()
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                g_items, (g_box, g_cls, g_ang) = crit(dbox, dcls, dang, dgl, dgb, dmk)
            for t in [g_items] + g_box + g_cls + g_ang:
                t.fill_(float("nan"))
            graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, [g_items] + g_box + g_cls + g_ang):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 6. DetectHead
def _bn_results(tag, blk):
    return {f"{tag}dW": blk.dw, f"{tag}dgamma": blk.dgamma, f"{tag}dbeta": blk.dbeta, f"{tag}rmean": blk.running_mean, f"{tag}rvar": blk.running_var}


def test_detect_head_matches_torch_modules_and_sgd():
    """One DetectHead.step at features 2x16x16x32, 2x8x8x64, 2x4x4x64, nc = 3: items, the three dx and every parameter gradient and running statistic
    within 2 e of the unrounded fp64 nn.Module stack under the same criterion (e = the reference's own rounded-against-plain distance, per tensor:
    criterion_ref.run_head), the assignment fed to the reference being the device's own; then the parameters after the SGD step against torch.optim
    fed the same gradients, within train_steps_ref.PARAM_TOL."""
    _ops()
    import oriented_object_detection_amd.train as TR
    from dw_ref import EPS, MOM, rel_dist
    from train_steps_ref import PARAM_TOL
    case = CR.head_case()
    levels, feats, (gl, gb, mk) = case
    dev = lambda m: tuple(t.clone().cuda() for t in m.init)
    lr, wd = 0.01, 5e-4
    spec = [{"box": ([dev(b)[:3] for b in lv["box"][0]], *dev(lv["box"][1])),
             "cls": ([(dev(dw), dev(pw)) for dw, pw in lv["cls"][0]], *dev(lv["cls"][1])),
             "angle": ([dev(b)[:3] for b in lv["angle"][0]], *dev(lv["angle"][1]))} for lv in levels]
    head = TR.DetectHead(spec, CR.HEAD_NC, optimizer="SGD", lr=lr, momentum=0.9, weight_decay=wd, eps=EPS, bn_momentum=MOM)
    pairs = []  # (tag, reference module, device module) in registration order
    mods = CR.head_modules(levels)
    devmods = []
    for i in range(3):
        devmods += head.box[i].blocks + [head.box[i]]
        devmods += [b for p in head.cls[i].pairs for b in (p.dw, p.pw)] + [head.cls[i].out]
        devmods += head.angle[i].blocks + [head.angle[i].out]
    assert len(devmods) == len(mods)
    for (tag, r), d in zip(mods, devmods):
        if hasattr(d, "running_mean"):
            d.running_mean.copy_(r.init[3]); d.running_var.copy_(r.init[4])
        pairs.append((tag, r, d))
    before = [t.clone() for t in head.groups.param]
    items, dx = head.step([x.cuda() for x in feats], gl.cuda(), gb.cuda(), mk.cuda())
    torch.cuda.synchronize()
    last = head.criterion.last
    assert int(last["fg_mask"].sum()) >= 8
    assign = (last["target_bboxes"].cpu(), last["target_scores"].cpu(), last["fg_mask"].cpu())
    got = {"items": items}
    for i in range(3):
        got[f"dx{i}"] = dx[i].double().cpu().permute(0, 3, 1, 2)
    for tag, r, d in pairs:
        if hasattr(d, "dgamma"):
            got.update(_bn_results(tag, d))
        elif hasattr(d, "dw3"):
            got.update({f"{tag}dW": d.dw3, f"{tag}db": d.db3})
        else:
            got.update({f"{tag}dW": d.dw, f"{tag}db": d.db})
    plain, rounded = CR.run_head(case, assign, False), CR.run_head(case, assign, True)
    assert set(got) == set(plain), set(got) ^ set(plain)
    worst = ("", 0.0)
    for n in plain:
        dist, e = rel_dist(got[n].cpu().reshape(plain[n].shape), plain[n]), rel_dist(rounded[n], plain[n])
        print(f"  DetectHead {n}: device {dist:.2e} (e {e:.2e})")
        worst = max(worst, (n, dist / e if e else float(dist > 0) * float("inf")), key=lambda t: t[1])
    print(f"  DetectHead worst distance / e: {worst[0]} {worst[1]:.3f}")
    assert worst[1] <= 2, worst
    # the SGD step against torch.optim on the same gradients
    params = [torch.nn.Parameter(t.cpu().clone()) for t in before]
    kinds = [g for g, _ in head.groups.items]
    topt = torch.optim.SGD([{"params": [p for p, k in zip(params, kinds) if k == j], "weight_decay": wd if j == 0 else 0.0} for j in range(3)], lr=lr,
                           momentum=0.9, nesterov=True, foreach=False)
    for p, gr in zip(params, head.groups.grad):
        p.grad = gr.cpu().clone()
    topt.step()
    for p, now in zip(params, head.groups.param):
        assert float((now.cpu() - p.detach()).abs().max()) <= PARAM_TOL * max(1.0, float(p.detach().abs().max()))
