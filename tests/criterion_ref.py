"""fp64 restatement of the fused OBB training criterion (csrc/criterion.hip; train.OBBCriterion) and its per-element bounds.  Used by
test_train_criterion_cpu.py (the restatement against oracle/postproc.decode, a hand-written chain rule, torch's own fp32 evaluation and planted
mistakes) and test_gpu_train_criterion.py (the device).  The criterion restates Ultralytics 8.3.x v8OBBLoss from recall (UNPINNED: the package is not
installed); it is built from torch ops plus oracle.loss.probiou (through train_loss_ref.probiou_mc, its operation-by-operation twin with rounding
hooks, checked against it in test_train_loss_cpu.py), oracle.loss.bce_loss / dfl_loss / rotated_tal_assign and oracle.yolo11_obb.make_anchors.
Gradients come from torch.autograd.

Bounds (the method of train_loss_ref / bounds.spread, its constants unchanged: FACTOR = 8, REL_MID = 2 u, THIN = 32, K = 8, inputs perturbed by 16 u):
  element bound = FACTOR x spread + floor;
  floor(gradient) = 8 u |ref| + 1e-30, + 2^-8 |ref| for the bf16-stored d_box, + the thin-box term THIN kappa u max_row |grad| and, where the
    ProbIoU clamp gate lies within its own error of either end, the open-gate gradient (both as train_loss_ref.probiou_bounds has them, applied to
    the anchor's whole row of logits: the chain rule spreads the pair's gradient over it);
  floor(loss item, tss) = (additions + 8) u sum |elements|, additions = the longest chain of additions an element passes through: 16 + 8 per level
    of the sum tree (16 strided values per thread, then the 256-wide tree), plus ceil(nc / 4) + 3 inside the per-anchor class / DFL elements.
No factor was changed by the CPU calibration (test_train_criterion_cpu.py prints the worst ratio of torch's fp32 evaluation per output)."""
import math

import torch
import torch.nn.functional as F

from bounds import U, spread
from oracle.yolo11_obb import make_anchors
from train_loss_ref import DFL_HI, FACTOR, PROBIOU_EPS, REL_MID, THIN, probiou_mc

REG_MAX = 16
STRIDES = (8, 16, 32)
GAINS = (7.5, 0.5, 1.5)

# (imgsz (H, W), B, nc, box dtype, seed) of the end-to-end cases: for each, the fp32 and the fp64 evaluation of oracle.loss.rotated_tal_assign agree
# on every discrete output (test_train_criterion_cpu.py::test_seeds_have_no_discrete_flip), so the GPU test excludes no anchor.
E2E_CASES = [
    ((128, 128), 2, 12, "bf16", 1),
    ((96, 160), 2, 15, "bf16", 2),
    ((96, 160), 1, 1, "fp32", 3),
    ((128, 128), 1, 15, "fp32", 4),
]


def level_shapes(imgsz):
    H, W = imgsz
    return [(H // s, W // s) for s in STRIDES]


def anchors(imgsz, dtype=torch.float64):
    """-> (anchor points [A,2] in grid units, strides [A]) from oracle.yolo11_obb.make_anchors"""
    pts, st = make_anchors(*imgsz)
    return pts.to(dtype), st.to(dtype)


def make_head(seed, imgsz, B, nc, box_dtype="bf16", scale=2.0):
    """random head logits per level, fp32 tensors holding the values the device reads (bf16 values for a bf16 box branch):
    -> (box [3 x [B,H,W,64]], cls [3 x [B,H,W,nc]], angle [3 x [B,H,W,1]])"""
    g = torch.Generator().manual_seed(seed)
    box, cls, ang = [], [], []
    for (h, w) in level_shapes(imgsz):
        b = torch.randn((B, h, w, 64), generator=g) * scale
        box.append(b.bfloat16().float() if box_dtype == "bf16" else b)
        cls.append(torch.randn((B, h, w, nc), generator=g) * 2.0 - 2.0)
        ang.append(torch.randn((B, h, w, 1), generator=g) * 1.5)
    return box, cls, ang


def make_gt(seed, imgsz, B, nc, n_max=8):
    """padded ground truth in pixels: between 0 and n_max boxes per image (image 0 always has some), sides 12 px .. half the image"""
    g = torch.Generator().manual_seed(1000 + seed)
    H, W = imgsz
    gl = torch.zeros((B, n_max), dtype=torch.int32)
    gb = torch.zeros((B, n_max, 5))
    mk = torch.zeros((B, n_max), dtype=torch.bool)
    for b in range(B):
        n = n_max - 2 * b
        r = torch.rand((n, 5), generator=g)
        gb[b, :n, 0] = (0.15 + 0.7 * r[:, 0]) * W
        gb[b, :n, 1] = (0.15 + 0.7 * r[:, 1]) * H
        gb[b, :n, 2] = 12 + r[:, 2] * (W / 2 - 12)
        gb[b, :n, 3] = 12 + r[:, 3] * (H / 2 - 12)
        gb[b, :n, 4] = (r[:, 4] - 0.25) * math.pi * 0.999
        gl[b, :n] = torch.randint(0, nc, (n,), generator=g).to(torch.int32)
        mk[b, :n] = True
    return gl, gb, mk


def cat_levels(ts, variant=""):
    """per-level [B,H,W,C] -> [B,A,C], anchors row-major, levels P3, P4, P5.  Planted mistakes: "swap_hw" walks each map column-major, "rev_levels"
    concatenates P5, P4, P3."""
    parts = [(t.transpose(1, 2) if variant == "swap_hw" else t).reshape(t.shape[0], -1, t.shape[-1]) for t in ts]
    return torch.cat(parts[::-1] if variant == "rev_levels" else parts, 1)


def split_levels(t, imgsz):
    """[B,A,C] -> per-level [B,H,W,C]"""
    out, o = [], 0
    for (h, w) in level_shapes(imgsz):
        out.append(t[:, o:o + h * w].reshape(t.shape[0], h, w, t.shape[-1]))
        o += h * w
    return out


def decode(box, ang, anc, rnd=lambda t: t, variant=""):
    """box [B,A,64], ang [B,A], anc [A,2] (grid units) -> (pred [B,A,5] in grid units, parts for the hand-written chain rule)"""
    B, A, _ = box.shape
    p = rnd(box.reshape(B, A, 4, REG_MAX).softmax(-1))
    E = rnd((p * torch.arange(REG_MAX, dtype=box.dtype)).sum(-1))
    l, t, r, b = E.unbind(-1)
    if variant == "swap_lt":
        l, t = t, l
    sig = rnd(torch.sigmoid(ang))
    th = rnd((sig - (0.0 if variant == "no_offset" else 0.25)) * math.pi)
    c, s = rnd(torch.cos(th)), rnd(torch.sin(th))
    xf, yf = rnd((r - l) / 2), rnd((b - t) / 2)
    x = rnd(anc[:, 0] + rnd(rnd(xf * c) - rnd(yf * s)))
    y = rnd(anc[:, 1] + rnd(rnd(xf * s) + rnd(yf * c)))
    w, h = rnd(l + r), rnd(t + b)
    return torch.stack([x, y, w, h, th], -1), dict(p=p, E=E, sig=sig, th=th, c=c, s=s, xf=xf, yf=yf)


def decode_px(box, cls, ang, imgsz):
    """the assigner's inputs in fp64 (or the dtype given): (pd_scores, pd_bboxes in pixels, anc_points in pixels, stride)"""
    anc, st = anchors(imgsz, box.dtype)
    pred, _ = decode(box, ang, anc)
    px = torch.cat([pred[..., :4] * st[None, :, None], pred[..., 4:]], -1)
    return torch.sigmoid(cls), px, anc * st[:, None], st


def target_ltrb(tg, anc, variant=""):
    """bbox2dist of grid-unit targets tg [n,5] against their anchors anc [n,2], clamped to [0, reg_max - 1 - 0.01] (the fp32 constant)"""
    x, y, w, h = tg[:, 0], tg[:, 1], tg[:, 2], tg[:, 3]
    d = torch.stack([anc[:, 0] - (x - w / 2), anc[:, 1] - (y - h / 2), (x + w / 2) - anc[:, 0], (y + h / 2) - anc[:, 1]], -1)
    return d.clamp(min=0) if variant == "no_clamp" else d.clamp(0, DFL_HI)


def dfl_rows(logits, ltrb):
    """DFLoss per anchor (oracle.loss.dfl_loss's formula, mean over the 4 sides, before weight and tss): logits [n,64], ltrb [n,4] clamped -> [n]"""
    tl = ltrb.long().clamp(max=REG_MAX - 1)
    tr = (tl + 1).clamp(max=REG_MAX - 1)
    wl = (tl + 1) - ltrb
    wr = 1 - wl
    pd = logits.reshape(-1, REG_MAX)
    ce = lambda idx: F.cross_entropy(pd, idx.reshape(-1), reduction="none").reshape(tl.shape)
    return (ce(tl) * wl + ce(tr) * wr).mean(-1)


def crit_total(box, cls, ang, tb, ts, fg, imgsz, gains=GAINS, rnd=lambda t: t, gate=True, variant=""):
    """the criterion of the issue's section 1, differentiable in box / cls / ang -> (items [3], tss, B * sum(items), braw, pred_fg, target_fg)"""
    dt = box.dtype
    B = box.shape[0]
    anc, st = anchors(imgsz, dt)
    pred, _ = decode(box, ang, anc, rnd, variant)
    s_all = ts.sum()
    tss = s_all if variant == "no_max" else s_all.clamp(min=1.0)
    bi, ai = fg.nonzero(as_tuple=True)
    weight = rnd(ts.sum(-1)[bi, ai])
    sdiv = torch.ones_like(st[ai]) if variant == "no_stride_div" else st[ai]
    tg = torch.cat([tb[bi, ai, :4] / sdiv[:, None], tb[bi, ai, 4:]], -1)
    pf = pred[bi, ai]
    if bi.numel():
        hd, braw = probiou_mc(pf, tg, rnd, gate=gate)
        l_box = rnd(hd * weight).sum() / tss
        l_dfl = rnd(rnd(dfl_rows(box[bi, ai], target_ltrb(tg, anc[ai], variant))) * weight).sum() / tss
    else:
        braw = torch.zeros(0, dtype=dt)
        l_box = l_dfl = box.sum() * 0
    l_cls = rnd(F.binary_cross_entropy_with_logits(cls, ts, reduction="none")).sum() / tss
    gb, gc, gd = gains
    if variant == "wrong_gain":
        gb, gc = gc, gb
    items = torch.stack([l_box * gb, l_cls * gc, l_dfl * gd])
    return items, tss, items.sum() * (1 if variant == "no_B" else B), braw, pf, tg


def crit_eval(box, cls, ang, tb, ts, fg, imgsz, gains=GAINS, rnd=lambda t: t, gate=True, variant=""):
    """crit_total in the dtype of its inputs (fp64 for the reference, fp32 for the calibration), gradients by autograd.
    box [B,A,64], cls [B,A,nc], ang [B,A]; tb [B,A,5] pixels, ts [B,A,nc], fg bool [B,A].
    -> dict(items [3], tss [1], d_box, d_cls, d_ang, braw [n_fg], pred [n_fg,5], tgt [n_fg,5])"""
    box, cls, ang = (t.detach().clone().requires_grad_(True) for t in (box, cls, ang))
    items, tss, total, braw, pf, tg = crit_total(box, cls, ang, tb, ts, fg, imgsz, gains, rnd, gate, variant)
    d_box, d_cls, d_ang = torch.autograd.grad(total, (box, cls, ang), allow_unused=True)
    z = lambda g, t: torch.zeros_like(t) if g is None else g
    return dict(items=items.detach(), tss=tss.detach().reshape(1), d_box=z(d_box, box), d_cls=z(d_cls, cls), d_ang=z(d_ang, ang), braw=braw.detach(),
                pred=pf.detach(), tgt=tg.detach())


def chain_rule(box, ang, gp, anc):
    """the hand-written chain rule of the issue's section 1, fp64: gp [B,A,5] = d L / d (x, y, w, h, theta) of the decoded box ->
    (d L / d box logits [B,A,64], d L / d angle logit [B,A]) through the decode alone"""
    pred, q = decode(box, ang, anc)
    gx, gy, gw, gh, gt = gp.unbind(-1)
    c, s, xf, yf = q["c"], q["s"], q["xf"], q["yf"]
    u = gx * c + gy * s
    v = -gx * s + gy * c
    dside = torch.stack([gw - u / 2, gh - v / 2, gw + u / 2, gh + v / 2], -1)
    dth = gt + gx * (-xf * s - yf * c) + gy * (xf * c - yf * s)
    da = dth * math.pi * q["sig"] * (1 - q["sig"])
    k = torch.arange(REG_MAX, dtype=box.dtype)
    dlog = q["p"] * (k - q["E"][..., None]) * dside[..., None]
    return dlog.reshape(box.shape), da


def depth(n, nc=0):
    """the longest chain of additions of n elements through the sum tree (+ the per-anchor element's own, see the module docstring)"""
    return 24 * (1 if n <= 4096 else 2) + (math.ceil(nc / 4) + 3 if nc else 0)


def crit_bounds(box, cls, ang, tb, ts, fg, imgsz, gains=GAINS, k=8, seed=0):
    """-> (ref dict of crit_eval in fp64, bound dict for items, tss, d_box, d_cls, d_ang, pd_scores, pd_bboxes) from fp32-valued inputs"""
    box, cls, ang, tb, ts = (t.double() for t in (box, cls, ang, tb, ts))
    keys = ("items", "tss", "d_box", "d_cls", "d_ang", "braw")

    def f(box, cls, ang, tb, ts, rnd):
        r = crit_eval(box, cls, ang, tb, ts, fg, imgsz, gains, rnd, gate=True)
        o = crit_eval(box, cls, ang, tb, ts, fg, imgsz, gains, rnd, gate=False)
        return tuple(r[k_] for k_ in keys) + (o["d_box"], o["d_ang"])

    base, sp = spread(f, [box, cls, ang, tb, ts], k=k, seed=seed, rel_mid=REL_MID)
    sp = [torch.nan_to_num(x, nan=float("inf")) for x in sp]
    ref = crit_eval(box, cls, ang, tb, ts, fg, imgsz, gains)
    B, A, nc = cls.shape
    bi, ai = fg.nonzero(as_tuple=True)
    braw, ob, oa = base[5], base[6], base[7]
    # per foreground anchor: the clamp gate and the thin-box term of train_loss_ref.probiou_bounds, spread over the anchor's row of logits
    row_extra = torch.zeros((B, A), dtype=torch.float64)
    near_full = torch.zeros((B, A), dtype=torch.bool)
    if bi.numel():
        db = FACTOR * sp[5] + 8 * U * braw.abs()
        near_full[bi, ai] = ((braw - PROBIOU_EPS).abs() <= db) | ((braw - 100.0).abs() <= db)
        wh = torch.cat([ref["pred"][:, 2:4], ref["tgt"][:, 2:4]], 1).abs()
        kappa = (wh[:, [0, 2]].maximum(wh[:, [1, 3]]) / wh[:, [0, 2]].minimum(wh[:, [1, 3]]).clamp_min(1e-30)).pow(2).amax(1)
        rowmax = torch.maximum(ref["d_box"][bi, ai].abs().amax(-1), ref["d_ang"][bi, ai].abs())
        row_extra[bi, ai] = THIN * kappa * U * rowmax
    gate_b = torch.where(near_full[..., None], ob.abs() + FACTOR * sp[6], torch.zeros_like(ob))
    gate_a = torch.where(near_full, oa.abs() + FACTOR * sp[7], torch.zeros_like(oa))
    n = B * A
    elems = torch.stack([ref["items"][0].abs(), ref["items"][1].abs(), ref["items"][2].abs()])  # all elements >= 0: sum |elements| = |item|
    bound = dict(
        items=FACTOR * sp[0] + torch.tensor([depth(n) + 8, depth(n, nc) + 8, depth(n, 16) + 8], dtype=torch.float64) * U * elems + 1e-30,
        tss=FACTOR * sp[1] + (depth(n * nc) + 8) * U * ts.abs().sum() + 1e-30,
        d_box=FACTOR * sp[2] + (8 * U + 2.0 ** -8) * ref["d_box"].abs() + 1e-30 + row_extra[..., None] + gate_b,
        d_cls=FACTOR * sp[3] + 8 * U * ref["d_cls"].abs() + 1e-30,
        d_ang=FACTOR * sp[4] + 8 * U * ref["d_ang"].abs() + 1e-30 + row_extra + gate_a,
    )
    return ref, bound


def decode_bounds(box, cls, ang, imgsz, k=8, seed=0):
    """-> ((pd_scores, pd_bboxes px) in fp64, their bounds): FACTOR x spread + 8 u |ref|"""
    box, cls, ang = (t.double() for t in (box, cls, ang))
    anc, st = anchors(imgsz)

    def f(box, cls, ang, rnd):
        pred, _ = decode(box, ang, anc, rnd)
        return rnd(torch.sigmoid(cls)), torch.cat([rnd(pred[..., :4] * st[None, :, None]), pred[..., 4:]], -1)

    (ps, pb), (s_ps, s_pb) = spread(f, [box, cls, ang], k=k, seed=seed, rel_mid=REL_MID)
    return (ps, pb), (FACTOR * s_ps + 8 * U * ps.abs() + 1e-30, FACTOR * s_pb + 8 * U * pb.abs() + 1e-30)


def hand_targets(seed, imgsz, B, nc, small_tss=False):
    """a hand-built assignment: foreground at the first and last anchor of every level and at random others; targets near their anchors, with
    targets hitting both ends of the ltrb clamp (an anchor far outside its box: sides < 0; a box far larger than 15 bins), thin boxes (60:1), and
    target scores summing below 1 (small_tss).  -> (tb [B,A,5] px, ts [B,A,nc], fg bool [B,A])"""
    g = torch.Generator().manual_seed(2000 + seed)
    anc, st = anchors(imgsz, torch.float32)
    A = anc.shape[0]
    fg = torch.rand((B, A), generator=g) < 0.08
    o = 0
    for (h, w) in level_shapes(imgsz):
        fg[:, o] = True
        fg[:, o + h * w - 1] = True
        o += h * w
    r = torch.rand((B, A, 5), generator=g)
    tb = torch.empty((B, A, 5))
    tb[..., 0] = (anc[:, 0] + (r[..., 0] - 0.5) * 3) * st
    tb[..., 1] = (anc[:, 1] + (r[..., 1] - 0.5) * 3) * st
    tb[..., 2] = (2 + r[..., 2] * 10) * st
    tb[..., 3] = (2 + r[..., 3] * 10) * st
    tb[..., 4] = (r[..., 4] - 0.25) * math.pi * 0.999
    tb[:, 0, :2] += 12 * st[0]          # anchor outside its box: left / top sides clamp at 0
    tb[:, 1, 2:4] = 40 * st[1]          # a box of 40 bins: every side clamps at 14.99
    tb[:, 2, 2] = 30 * st[2]; tb[:, 2, 3] = 0.5 * st[2]  # thin, 60:1
    fg[:, :3] = True
    ts = torch.zeros((B, A, nc))
    lab = torch.randint(0, nc, (B, A), generator=g)
    val = torch.rand((B, A), generator=g) * (0.002 if small_tss else 0.9) + (0.0 if small_tss else 0.05)
    ts.scatter_(2, lab[..., None], val[..., None])
    ts = ts * fg[..., None]
    return tb, ts, fg


# ---------------------------------------------------------------------------------------------- the three-level head under the criterion
HEAD_FEATS = [(2, 16, 16, 32), (2, 8, 8, 64), (2, 4, 4, 64)]  # imgsz 128: P3, P4, P5 features, NHWC
HEAD_NC, HEAD_C2, HEAD_C3, HEAD_C4 = 3, 16, 16, 8             # classes; widths of the box, class and angle branches


def head_case(seed=0):
    """-> (levels, feats, gt): per level {"box": (blocks, head), "cls": (pairs, head), "angle": (blocks, head)} of dw_ref.RefBlock / narrow_ref.RefHead
    (the fp64 nn.Module stacks of Detect.cv2 / cv3 / OBB.cv4), bf16 features, the padded ground truth"""
    from dw_ref import RefBlock
    from narrow_ref import RefHead
    g = torch.Generator().manual_seed(4242 + seed)
    levels, feats = [], []
    for (B, H, W, c) in HEAD_FEATS:
        levels.append({
            "box": ([RefBlock(g, c, HEAD_C2, 3, 1, True), RefBlock(g, HEAD_C2, HEAD_C2, 3, 1, True)], RefHead(g, HEAD_C2, 64)),
            "cls": ([(RefBlock(g, c, c, 3, c, True), RefBlock(g, c, HEAD_C3, 1, 1, True)),
                     (RefBlock(g, HEAD_C3, HEAD_C3, 3, HEAD_C3, True), RefBlock(g, HEAD_C3, HEAD_C3, 1, 1, True))], RefHead(g, HEAD_C3, HEAD_NC)),
            "angle": ([RefBlock(g, c, HEAD_C4, 3, 1, True), RefBlock(g, HEAD_C4, HEAD_C4, 3, 1, True)], RefHead(g, HEAD_C4, 1)),
        })
        feats.append(torch.randn(B, H, W, c, generator=g).to(torch.bfloat16))
    return levels, feats, make_gt(seed, (128, 128), 2, HEAD_NC)


def head_modules(levels):
    """[(tag, module)] in the order train.DetectHead registers them"""
    out = []
    for i, lv in enumerate(levels):
        out += [(f"l{i}.box.c{j}.", b) for j, b in enumerate(lv["box"][0])] + [(f"l{i}.box.out.", lv["box"][1])]
        out += [(f"l{i}.cls.p{j}.{n}.", b) for j, p in enumerate(lv["cls"][0]) for n, b in zip(("dw", "pw"), p)] + [(f"l{i}.cls.out.", lv["cls"][1])]
        out += [(f"l{i}.angle.c{j}.", b) for j, b in enumerate(lv["angle"][0])] + [(f"l{i}.angle.out.", lv["angle"][1])]
    return out


def run_head(case, assignment, rounded, gains=GAINS):
    """The stack PLAIN or ROUNDED to bf16 at the device's rounding points (dw_ref's scheme; the box branch's 64 logits and their gradient are bf16 on
    the device, the class and angle logits fp32), under crit_total with the given assignment (tb, ts, fg) -> {name: tensor}: items, dx per level and
    every parameter gradient and running statistic."""
    from dw_ref import _GradBf16, _q
    levels, feats, _ = case
    tb, ts, fg = assignment
    mods = head_modules(levels)
    for _, m in mods:
        m.reset()
    xs, outs = [], ([], [], [])
    for lv, x in zip(levels, feats):
        xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        xs.append(xr)
        a = xr
        for b in lv["box"][0]:
            a = b(a, rounded)
        y = lv["box"][1](a, rounded)
        outs[0].append(_GradBf16.apply(_q(y)) if rounded else y)
        a = xr
        for p in lv["cls"][0]:
            for b in p:
                a = b(a, rounded)
        outs[1].append(lv["cls"][1](a, rounded))
        a = xr
        for b in lv["angle"][0]:
            a = b(a, rounded)
        outs[2].append(lv["angle"][1](a, rounded))
    nhwc = lambda ts_: cat_levels([t.permute(0, 2, 3, 1) for t in ts_])
    items, tss, total, _, _, _ = crit_total(nhwc(outs[0]), nhwc(outs[1]), nhwc(outs[2])[..., 0], tb.double(), ts.double(), fg, (128, 128), gains)
    total.backward()
    res = {"items": items.detach().clone()}
    for i, xr in enumerate(xs):
        res[f"dx{i}"] = xr.grad.clone()
    for tag, m in mods:
        res.update(m.results(tag))
    return res
