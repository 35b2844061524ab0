"""fp64 reference of the post-processing chain (csrc/decode.hip: decode, ProbIoU Fast-NMS, result rows), written from the Ultralytics
semantics as oracle/postproc.py and SURVEY.md Appendix A2/A4/A6 restate them -- not from the kernels: no far-apart test, no fast-decision
band, no class skip; every pair is evaluated, cross-class pairs included, with the class offset of 7680 at every threshold.
Used by test_postproc_ref_cpu.py (the reference against the fp32 oracle, its mutations, the committed inputs) and by
test_gpu_postproc_elems.py (the kernels against it).  u = 2^-24.

Bounds.  decode_bounds derives E per element by counting the fp32 roundings of the restated formula on the term magnitudes, with L_ULP
units in the last place for expf / cosf / sinf (no accuracy table of the device library ships with the toolchain; the host's fp32 torch
evaluation measures a worst |err| / E of 0.47 on the decode inputs and 0.40 .. 0.55 on the NMS cases, test_postproc_ref_cpu.py; the device
measures 0.42 .. 0.55: 4 ulp is tighter than four times the host's error and leaves the device its few ulp of difference), and never below the Monte-Carlo-arithmetic floor of bounds.spread (the head is exact input: only the intermediates are
perturbed, by REL_MID).

Decisions.  nms_prepare evaluates one image: candidates, stable order, all-pairs ProbIoU with a floor per pair (bounds.spread over
train_loss_ref.probiou_mc: the decoded boxes perturbed by 16 u, every intermediate -- the class-offset add included -- by REL_MID) and a
report of what is decided: a comparison a >= b is decided when |a - b| > MARGIN x its floor.  A case whose pair decisions, confidence
thresholds, first-maximum classes and confidence order are all decided has ONE correct output: every correct fp32 implementation must
produce the same rows in the same order.  Synth draws inputs (boxes clustered on a few objects, classes biased towards two or three)
and re-draws the head rows that take part in an undecided comparison until none is left; it never looks at a device result.  That
search takes minutes, so its outcome (how often each row was redrawn) is committed as tests/golden/postproc_attempts.json by
tests/golden/make_postproc_attempts.py; the tests rebuild the heads from it and prove decidedness again in ONE evaluation per image.

Limits: every box is kept above 1 px (the far-apart bound of decode.hip assumes the log term of the Bhattacharyya distance >= 0, which the
eps of its denominator breaks far below a tenth of a pixel); nc <= 80."""
import json
import math
import os

import numpy as np
import torch

from bounds import U, spread
from train_loss_ref import FACTOR, REL_MID, probiou_mc

MARGIN = FACTOR      # a comparison is decided when the distance exceeds MARGIN x the floor of its operands
L_ULP = 4.0          # expf / cosf / sinf: units in the last place allowed to the device library
MAX_WH = 7680.0
THRESHOLDS = (5e-4, 0.1, 0.45, 0.7, 0.9)
PI32 = float(np.float32(math.pi))          # what `tensor % math.pi` uses on an fp32 tensor
HALF_PI32 = float(np.float32(math.pi / 2))
_id = lambda t: t

MUTATIONS = ("no_offset", "gt", "last_max", "tie_desc", "greedy", "maxdet_first", "angle_half", "wh_swap", "stride_shift")


def no_of(nc):
    return (64 + nc + 1 + 3) // 4 * 4


def f32v(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------- decode
def anchors(h, w, shift=0):
    """anchor centres [A,2] (grid units, +0.5) and strides [A], P3 P4 P5 row-major; shift rotates the level-to-stride table (a mutation)"""
    table = (8, 16, 32)
    pts, st = [], []
    for l, s in enumerate(table):
        hh, ww = h // s, w // s
        yy, xx = torch.meshgrid(torch.arange(hh, dtype=torch.float64) + 0.5, torch.arange(ww, dtype=torch.float64) + 0.5, indexing="ij")
        pts.append(torch.stack((xx, yy), -1).reshape(-1, 2))
        st.append(torch.full((hh * ww,), float(table[(l + shift) % 3]), dtype=torch.float64))
    return torch.cat(pts), torch.cat(st)


def _sigmoid(x, rnd=_id):
    return rnd(1.0 / rnd(1.0 + rnd(torch.exp(-x))))


def decode64(head, h, w, nc, rnd=_id, mut=None, parts=False):
    """head [B,A,>=64+nc+1] (fp64 values of the fp32 logits) -> [B,A,4+nc+1] (x, y, w, h, class scores, theta)"""
    B, A, _ = head.shape
    anc, st = anchors(h, w, 1 if mut == "stride_shift" else 0)
    x = head[..., :64].reshape(B, A, 4, 16)
    z = rnd(x - x.amax(-1, keepdim=True))
    e = rnd(torch.exp(z))
    p = rnd(e / rnd(e.sum(-1, keepdim=True)))
    k = torch.arange(16, dtype=torch.float64)
    d = rnd(rnd(p * k).sum(-1))                                                   # [B,A,4] l, t, r, b
    sig = _sigmoid(head[..., 64 + nc], rnd)
    ang = rnd(rnd(sig - (0.5 if mut == "angle_half" else 0.25)) * math.pi)
    c, s = rnd(torch.cos(ang)), rnd(torch.sin(ang))
    xf, yf = rnd(rnd(d[..., 2] - d[..., 0]) / 2), rnd(rnd(d[..., 3] - d[..., 1]) / 2)
    xr, yr = rnd(rnd(xf * c) - rnd(yf * s)), rnd(rnd(xf * s) + rnd(yf * c))
    ox, oy = rnd(rnd(xr + anc[:, 0]) * st), rnd(rnd(yr + anc[:, 1]) * st)
    ow, oh = rnd(rnd(d[..., 0] + d[..., 2]) * st), rnd(rnd(d[..., 1] + d[..., 3]) * st)
    cls = _sigmoid(head[..., 64:64 + nc], rnd)
    out = torch.cat([torch.stack([ox, oy, ow, oh], -1), cls, ang[..., None]], -1)
    if parts:
        return out, dict(z=z, p=p, d=d, sig=sig, ang=ang, c=c, s=s, xf=xf, yf=yf, xr=xr, yr=yr, anc=anc, st=st)
    return out


def decode_bounds(head32, h, w, nc):
    """-> (fp64 decode of the fp32 head, E per element).  Roundings counted on the restated formula (u each, L_ULP u for libm):
      e_k = exp(x_k - m): relative (|x_k - m| + L) u           (the subtraction's rounding enters the exponent; exp(0) = 1 is exact)
      d = sum_k p_k k, p = e / sum e: sum_k p_k |k - d| relerr(e_k)  (a common factor of all e_k cancels)  + 32 u d  (15 adds of the
          denominator, the division, the product with k, 15 adds of the expectation)
      sigmoid: (L + 2) u sig;  theta = (sig - 0.25) pi: (L + 2) u sig pi + 2.5 u |theta|  (subtraction, product, fp32(pi) against pi)
      cos, sin: L u + the other one times E_theta;   xf = (r - l) / 2: (E_l + E_r) / 2 + u |xf|
      x = xf c - yf s: operands' errors on the partner's magnitude + u (|xf c| + |yf s| + |x|);  (x + ax) stride: + u |x + ax|, + u |out|
      w = (l + r) stride: (E_l + E_r + u (l + r)) stride + u |w|
    and never below the spread floor of decode64 with every intermediate perturbed by REL_MID (8 draws)."""
    hd = head32.double()
    ref, q = decode64(hd, h, w, nc, parts=True)
    u = U
    k = torch.arange(16, dtype=torch.float64)
    rel_e = torch.where(q["z"] == 0, torch.zeros_like(q["z"]), (q["z"].abs() + L_ULP) * u)
    Ed = (q["p"] * (k - q["d"][..., None]).abs() * rel_e).sum(-1) + 32 * u * q["d"] + 120 * 2.0 ** -126  # (+ every e_k flushed to zero below 2^-126)
    Eang = (L_ULP + 2) * u * q["sig"] * math.pi + 2.5 * u * q["ang"].abs()
    Ec, Es = L_ULP * u * q["c"].abs() + q["s"].abs() * Eang, L_ULP * u * q["s"].abs() + q["c"].abs() * Eang
    Exf = (Ed[..., 0] + Ed[..., 2]) / 2 + u * q["xf"].abs()
    Eyf = (Ed[..., 1] + Ed[..., 3]) / 2 + u * q["yf"].abs()
    xf, yf, c, s = q["xf"].abs(), q["yf"].abs(), q["c"].abs(), q["s"].abs()
    Exr = Exf * c + xf * Ec + Eyf * s + yf * Es + u * (xf * c + yf * s + q["xr"].abs())
    Eyr = Exf * s + xf * Es + Eyf * c + yf * Ec + u * (xf * s + yf * c + q["yr"].abs())
    st, anc = q["st"], q["anc"]
    Eox = (Exr + u * (q["xr"] + anc[:, 0]).abs()) * st + u * ref[..., 0].abs()
    Eoy = (Eyr + u * (q["yr"] + anc[:, 1]).abs()) * st + u * ref[..., 1].abs()
    Eow = (Ed[..., 0] + Ed[..., 2] + u * (q["d"][..., 0] + q["d"][..., 2])) * st + u * ref[..., 2].abs()
    Eoh = (Ed[..., 1] + Ed[..., 3] + u * (q["d"][..., 1] + q["d"][..., 3])) * st + u * ref[..., 3].abs()
    Ecls = (L_ULP + 2) * u * ref[..., 4:4 + nc] + 2.0 ** -149
    E = torch.cat([torch.stack([Eox, Eoy, Eow, Eoh], -1), Ecls, Eang[..., None]], -1)
    _, floor = spread(lambda t, rnd: decode64(t, h, w, nc, rnd), [hd], rel=0.0, rel_mid=REL_MID)
    return ref, torch.maximum(E, floor)


# ---------------------------------------------------------------------------------------------- NMS
def _pairs_iou(boxes, cls, I, J, rnd=_id, mut=None):
    """ProbIoU of the pairs (I, J) of decoded boxes [n,5] with the class offset added to the centres (one fp32 rounding each)"""
    b = boxes
    if mut == "wh_swap":
        b = torch.stack([b[:, 0], b[:, 1], b[:, 3], b[:, 2], b[:, 4]], -1)
    off = cls.double() * (0.0 if mut == "no_offset" else MAX_WH)
    b = torch.stack([rnd(b[:, 0] + off), rnd(b[:, 1] + off), b[:, 2], b[:, 3], b[:, 4]], -1)
    hd, _ = probiou_mc(b[I], b[J], rnd)
    return 1.0 - hd


class Case:
    """one image through the reference: everything that does not depend on (iou_thres, max_det)"""
    pass


def nms_prepare(head32, h, w, nc, conf_thres, max_nms=30000, mut=None, floors=True, window=None, margin=None):
    """head32 [A, >=64+nc+1] fp32 of ONE image -> Case: candidates in score order, pair IoUs (+ floors), decidedness of the candidate set."""
    margin = MARGIN if margin is None else margin
    hd = head32.double()[None]
    pred = decode64(hd, h, w, nc, mut=mut)[0]
    A = pred.shape[0]
    logits = hd[0, :, 64:64 + nc]
    scores = pred[:, 4:4 + nc]
    if mut == "last_max":
        best = scores.amax(1)
        j = (nc - 1) - torch.flip(scores, (1,)).argmax(1)
    else:
        best = scores.amax(1)  # the FIRST maximum is the class
        j = torch.where(scores == best[:, None], torch.arange(nc)[None].expand(A, nc), torch.full((A, nc), nc)).amin(1)
    ct = f32v(conf_thres)
    cand = torch.nonzero(best > ct)[:, 0]
    c = Case()
    c.A, c.nc, c.conf_thres, c.pred = A, nc, ct, pred
    conf = best[cand]
    if mut == "tie_desc":  # equal confidences in descending anchor order
        o = (len(conf) - 1 - torch.argsort(torch.flip(conf, (0,)), descending=True, stable=True))
    else:
        o = torch.argsort(conf, descending=True, stable=True)
    o = o[:max_nms]
    c.anchor = cand[o]
    c.conf, c.cls = conf[o], j[cand][o]
    c.box = torch.cat([pred[c.anchor, :4], pred[c.anchor, 4 + nc:]], -1)
    n = len(o)
    c.n = n
    c.I, c.J = torch.triu_indices(n, n, 1)
    if floors and n > 1 and window is not None:
        # large cases: the floor is evaluated for the pairs within window[0] of one of the thresholds window[1] only (the others keep
        # floor 0); the largest floor found must stay below a quarter of the window over MARGIN, or the short cut is refused
        c.iou = _pairs_iou(c.box, c.cls, c.I, c.J)
        sel = torch.zeros(len(c.iou), dtype=torch.bool)
        for t in window[1]:
            sel |= (c.iou - f32v(t)).abs() < window[0]
        Is, Js = c.I[sel], c.J[sel]
        _, fl = spread(lambda b, k, rnd: _pairs_iou(b, k, Is, Js, rnd), [c.box, c.cls], rel_mid=REL_MID)
        assert not len(fl) or MARGIN * float(fl.max()) < window[0] / 4, float(fl.max())
        c.iou_floor = torch.zeros_like(c.iou)
        c.iou_floor[sel] = fl
    elif floors and n > 1:
        f = lambda b, k, rnd: _pairs_iou(b, k, c.I, c.J, rnd, mut)
        c.iou, c.iou_floor = spread(f, [c.box, c.cls], rel_mid=REL_MID)
    else:
        c.iou = _pairs_iou(c.box, c.cls, c.I, c.J, mut=mut) if n > 1 else torch.zeros(0, dtype=torch.float64)
        c.iou_floor = torch.zeros_like(c.iou)
    if not floors:
        return c
    # ---- decidedness of the candidate set (independent of the IoU threshold): anchors listed in c.bad_anchors take part in an undecided comparison
    srt, _ = torch.sort(logits, 1, descending=True)
    top = srt[:, 0]
    _, fl = spread(lambda t, rnd: _sigmoid(t, rnd), [top], rel=0.0, rel_mid=REL_MID)
    fl = fl + 2.0 ** -149
    s_top = torch.sigmoid(top)
    und_conf = (s_top - ct).abs() <= margin * fl
    und_cls = torch.zeros(A, dtype=torch.bool)
    if nc > 1:
        run = srt[:, 1]
        und_cls = ((s_top - torch.sigmoid(run)) <= margin * 2 * fl) & (run != top) & (best > ct)
    # confidence order: neighbours in the sorted list are separated, or come from bit-identical class rows
    und_tie = torch.zeros(A, dtype=torch.bool)
    if n > 1:
        d = c.conf[:-1] - c.conf[1:]
        same = (logits[c.anchor[:-1]] == logits[c.anchor[1:]]).all(1)
        und = (d <= margin * 2 * fl[c.anchor[1:]]) & ~same
        und_tie[c.anchor[1:][und]] = True
    c.n_und_conf, c.n_und_cls, c.n_und_tie = int(und_conf.sum()), int(und_cls.sum()), int(und_tie.sum())
    c.bad_anchors = set(torch.nonzero(und_conf | und_cls | und_tie)[:, 0].tolist())
    return c


def nms_run(c, iou_thres, max_det, mut=None, exact=False):
    """-> (rows [m,7] (x, y, w, h, conf, cls, theta) fp64, kept positions in the sorted candidate list, number of suppressed rows).
    exact: the threshold is taken as the fp64 value given, not rounded to fp32 (to put it onto a pair's own IoU)"""
    thr = float(iou_thres) if exact else f32v(iou_thres)
    n = c.n
    if mut == "maxdet_first":
        n = min(n, max_det)
    sel = (c.J < n)
    hit = (c.iou > thr) if mut == "gt" else (c.iou >= thr)
    hit = hit & sel
    if mut == "greedy":  # a suppressed row no longer suppresses
        M = torch.zeros((n, n), dtype=torch.bool)
        M[c.I[hit], c.J[hit]] = True
        alive = torch.ones(n, dtype=torch.bool)
        for i in range(n):
            if alive[i]:
                alive &= ~M[i]
        supp = ~alive
    else:
        supp = torch.zeros(n, dtype=torch.bool)
        supp[c.J[hit]] = True
    kept = torch.nonzero(~supp)[:, 0]
    nsupp = int(supp.sum())
    kept = kept[:max_det]
    rows = torch.cat([c.box[kept, :4], c.conf[kept, None], c.cls[kept, None].double(), c.box[kept, 4:]], -1)
    return rows, kept, nsupp


def list_case(box32, score32):
    """Case of a caller-provided candidate list (boxes [n,5] with any class offset already applied, scores [n]): k_probiou_nms_list"""
    c = Case()
    c.order = torch.argsort(score32.double(), descending=True, stable=True)
    c.anchor, c.n = c.order, len(c.order)
    c.box, c.conf, c.cls = box32.double()[c.order], score32.double()[c.order], torch.zeros(c.n, dtype=torch.long)
    c.I, c.J = torch.triu_indices(c.n, c.n, 1)
    if c.n > 1:
        c.iou, c.iou_floor = spread(lambda b, k, rnd: _pairs_iou(b, k, c.I, c.J, rnd), [c.box, c.cls], rel_mid=REL_MID)
    else:
        c.iou = c.iou_floor = torch.zeros(0, dtype=torch.float64)
    return c


def pair_report(c, iou_thres, margin=MARGIN):
    """-> dict: undecided pairs at this threshold (positions J of the later row), the tightest decided margin |iou - thr| / floor, and
    the populations of the pruning branches computed from their documented formulas in fp64 (properties of the inputs)"""
    thr = f32v(iou_thres)
    dist = (c.iou - thr).abs()
    und = dist <= margin * c.iou_floor
    ratio = torch.where(c.iou_floor > 0, dist / c.iou_floor.clamp_min(1e-300), torch.full_like(dist, float("inf")))
    rep = {"n_und_pairs": int(und.sum()), "bad_rows": set(c.anchor[c.J[und]].tolist()), "margin": float(ratio.min()) if len(ratio) else float("inf")}
    s = 1.0 + 1e-7 - (1.0 - thr) ** 2
    if thr > 1e-3 and 0 < s < 1 and c.n > 1:
        bdmax = -math.log(s)
        b, I, J = c.box, c.I, c.J
        same = c.cls[I] == c.cls[J]
        tr = (b[:, 2] ** 2 + b[:, 3] ** 2) / 12
        d2 = (b[I, 0] - b[J, 0]) ** 2 + (b[I, 1] - b[J, 1]) ** 2
        far = d2 > 4 * bdmax * 1.05 * (tr[I] + tr[J])
        bd = -torch.log((1.0 + 1e-7 - (1.0 - c.iou) ** 2).clamp_min(1e-300))  # the distance this IoU comes from (monotone)
        band = (bd - bdmax).abs() <= 1e-4 + 1e-3 * bdmax
        rep.update(far=int((same & far).sum()), near=int((same & ~far).sum()), band=int((same & ~far & band).sum()))
    return rep


# ---------------------------------------------------------------------------------------------- inputs
def favoured(nc):
    return sorted({0, min(1, nc - 1), nc - 1})


class Synth:
    """Synthetic head [B, A, no(nc)] for decode + NMS: per image a few objects; every anchor regresses one of them with a jitter of
    1 % .. 30 % (DFL logits concentrated on the two bins around each side, angle logit from the object's angle), so same-class neighbours
    overlap at every IoU; `ncand[b]` anchors get a class logit above logit(conf) (one of the favoured classes, half of them with a
    runner-up class), all others stay below.  `ties`: blocks of 4 consecutive anchors that share one bit-identical row.
    Row (b, a) is a pure function of (seed, b, a, attempt[b, a]): redraw() bumps the attempt of the rows it is given."""

    def __init__(self, h, w, nc, ncand, conf, seed, ties=0, nobj=5, ang_logit=None, dup_max=False, attempts=()):
        self.ang_logit, self.dup_max = ang_logit, dup_max
        self.h, self.w, self.nc, self.ncand, self.conf, self.seed = h, w, nc, list(ncand), conf, seed
        self.B = len(ncand)
        anc, st = anchors(h, w)
        self.anc, self.st = anc.numpy(), st.numpy()
        self.A = len(self.st)
        self.fav = favoured(nc)
        self.L = math.log(conf / (1 - conf))
        self.attempt = np.zeros((self.B, self.A), np.int64)
        for b, a, k in attempts:  # the committed result of the search (tests/golden/postproc_attempts.json)
            self.attempt[b, a] = k
        self.head = np.zeros((self.B, self.A, no_of(nc)), np.float32)
        self.src = np.tile(np.arange(self.A), (self.B, 1))  # the anchor whose row this anchor carries
        self.is_cand = np.zeros((self.B, self.A), bool)
        self.objs = []
        for b in range(self.B):
            g = np.random.default_rng([seed, b, 1 << 20])
            m = min(h, w)
            self.objs.append(dict(c=g.uniform(0.2, 0.8, (nobj, 2)) * (w, h), wh=g.uniform(0.12, 0.4, (nobj, 2)) * m,
                                  t=g.uniform(-0.7, 2.2, nobj), k=g.choice(self.fav, nobj)))
            tied = np.zeros(self.A, bool)
            for t in range(ties):  # (inside one level: P3 rows)
                a0 = int(g.integers(0, (h // 8) * (w // 8) - 4))
                self.src[b, a0:a0 + 4] = a0
                tied[a0:a0 + 4] = True
            if self.ncand[b] >= 8:  # tie blocks are candidates wherever the image has room for them
                self.is_cand[b, tied] = True
            free = g.permutation(np.nonzero(~tied)[0])
            self.is_cand[b, free[:self.ncand[b] - int(self.is_cand[b].sum())]] = True
            for a in range(self.A):
                if self.src[b, a] == a:
                    self._row(b, a)
            self.head[b] = self.head[b, self.src[b]]

    def _row(self, b, a):
        g = np.random.default_rng([self.seed, b, a, int(self.attempt[b, a])])
        o = self.objs[b]
        i = int(g.integers(0, len(o["k"])))
        sc = float(g.choice([0.01, 0.03, 0.1, 0.3]))
        cxy = o["c"][i] + sc * o["wh"][i] * g.standard_normal(2)
        wh = o["wh"][i] * np.exp(sc * g.standard_normal(2))
        th = float(np.clip(o["t"][i] + 0.5 * sc * g.standard_normal(), -0.78, 2.35))
        s = self.st[a]
        dx, dy = cxy[0] / s - self.anc[a, 0], cxy[1] / s - self.anc[a, 1]
        xf, yf = dx * math.cos(th) + dy * math.sin(th), -dx * math.sin(th) + dy * math.cos(th)
        ltrb = np.clip([wh[0] / s / 2 - xf, wh[1] / s / 2 - yf, wh[0] / s / 2 + xf, wh[1] / s / 2 + yf], 0.3, 14.7)
        row = self.head[b, a]
        row[:] = 0
        dfl = g.normal(-8.0, 1.0, (4, 16))
        for q in range(4):
            k0 = int(math.floor(ltrb[q])); f = ltrb[q] - k0
            dfl[q, k0], dfl[q, k0 + 1] = 4 + math.log(1 - f + 1e-3), 4 + math.log(f + 1e-3)
        row[:64] = dfl.reshape(-1)
        p = th / math.pi + 0.25
        row[64 + self.nc] = math.log(p / (1 - p)) if self.ang_logit is None else self.ang_logit
        cl = g.uniform(-12.0, self.L - 1.5 if self.L - 1.5 > -12 else -11.9, self.nc)
        cl = np.minimum(cl, self.L - 0.3)
        k = int(o["k"][i]) if g.random() < 0.75 else int(g.choice(self.fav))
        if self.is_cand[b, a]:
            cl[k] = self.L + g.uniform(0.05, 3.0)
            if g.random() < 0.5 and len(self.fav) > 1:
                k2 = int(g.choice([c for c in self.fav if c != k]))
                cl[k2] = cl[k] - g.uniform(0.3, 2.0)
                if self.dup_max and g.random() < 0.3:
                    cl[k2] = cl[k]  # two bit-identical maxima: the first one is the class
        else:
            cl[k] = self.L - g.uniform(0.05, 3.0)
        row[64:64 + self.nc] = cl

    def redraw(self, b, anchors_):
        for a in sorted({int(self.src[b, a]) for a in anchors_}):
            self.attempt[b, a] += 1
            self._row(b, a)
        self.head[b] = self.head[b, self.src[b]]

    def tensor(self):
        return torch.from_numpy(self.head.copy())


def decided_cases(syn, thresholds=THRESHOLDS, max_rounds=1, window=None, margin=MARGIN):
    """-> list of Case (one per image of `syn`), each fully decided at every threshold.  max_rounds = 1 (the tests): ONE evaluation of
    the head as it stands, an undecided comparison raises.  More rounds (make_postproc_attempts.py): rows that take part in an undecided
    comparison are redrawn until none is left; raises if that does not converge: change the seed."""
    cases = [None] * syn.B
    for b in range(syn.B):
        for rnd_ in range(max_rounds):
            c = nms_prepare(torch.from_numpy(syn.head[b]), syn.h, syn.w, syn.nc, syn.conf, window=None if window is None else (window, thresholds),
                            margin=margin)
            bad = set(c.bad_anchors)
            for t in thresholds:
                bad |= pair_report(c, t, margin)["bad_rows"]
            if not bad:
                break
            syn.redraw(b, bad)
        else:
            raise AssertionError(f"image {b}: undecided comparisons left after {max_rounds} evaluation(s) (seed {syn.seed}, anchors {sorted(bad)[:8]})")
        assert c.n == syn.ncand[b], (b, c.n, syn.ncand[b])
        cases[b] = c
    return cases


def assert_decided(c, thresholds):
    """the cap on undecided pairs, candidates and ties is zero"""
    assert (c.n_und_conf, c.n_und_cls, c.n_und_tie) == (0, 0, 0), (c.n_und_conf, c.n_und_cls, c.n_und_tie)
    for t in thresholds:
        assert pair_report(c, t)["n_und_pairs"] == 0, t


# The committed NMS matrix (test_postproc_ref_cpu.py checks every entry; test_gpu_postproc_elems.py runs the kernels on them).
NMS_NC = (1, 12, 16, 17, 80)
NMS_CONF = (0.25, 0.6, 0.001)
NMS_MAX_DET = (5, 40, 300)
NMS_TILES = (0, 1, 40, 256, 257, 330)   # candidates per image of the 128 x 128 batch (336 anchors): 256 | 257 is kCandCap's hand-over
_CACHE = {}
ATTEMPTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postproc_attempts.json")
SEARCH = {"on": False, "found": {}}   # make_postproc_attempts.py switches the search on and collects the tables
SEARCH_MARGIN = 1.05 * MARGIN          # the search keeps 5 % of reserve, so that another libm's last bit cannot undecide a committed case


def _table():
    if "table" not in _CACHE:
        _CACHE["table"] = json.load(open(ATTEMPTS)) if os.path.exists(ATTEMPTS) else {}
    return _CACHE["table"]


def _case(key, make, thresholds, window=None):
    """The committed case `key`: make(attempts) -> Synth with the redraw counts of the committed table, proved decided by one evaluation.
    The search for that table (redrawing undecided rows, minutes of CPU) runs only from make_postproc_attempts.py."""
    if key not in _CACHE:
        if SEARCH["on"]:
            syn = make(())
            cases = decided_cases(syn, thresholds, 40, window, SEARCH_MARGIN)
            SEARCH["found"][key] = [[int(b), int(a), int(syn.attempt[b, a])] for b, a in zip(*np.nonzero(syn.attempt))]
        else:
            assert key in _table(), f"{key}: not in {ATTEMPTS}; run tests/golden/make_postproc_attempts.py"
            syn = make(_table()[key])
            cases = decided_cases(syn, thresholds, 1, window)
        _CACHE[key] = (syn, cases)
    return _CACHE[key]


def nms_matrix_case(nc, conf):
    """-> (Synth, [Case per image]) of the 128 x 128 batch for (nc, conf), decided at all five thresholds; two tie blocks per image.
    The three conf values of one nc share the seed: the same boxes and IoUs, only the class logits move with logit(conf) -- they add
    the conf decisions and the round form of conf 0.001, not geometric variety (that comes from the five nc)."""
    return _case(f"matrix nc {nc} conf {conf}", lambda at: Synth(128, 128, nc, NMS_TILES, conf, seed=1000 + nc, ties=2, attempts=at), THRESHOLDS)


BIG = {"640": (0.7,), "416": (0.45, 0.7)}


def big_case(which):
    """"640": 640 x 640, B = 1, about 1500 candidates (the three-kernel fall-back);  "416": 416 x 416, B = 2 (the LDS-resident
    all-rows form).  nc = 12, conf 0.25, decided at iou 0.7 (and 0.45 for the 416 case); pair floors within 0.02 of those only."""
    if which == "640":
        make = lambda at: Synth(640, 640, 12, (1500,), 0.25, seed=7, nobj=40, attempts=at)
    else:
        make = lambda at: Synth(416, 416, 12, (700, 300), 0.25, seed=8, nobj=20, attempts=at)
    return _case(f"big {which}", make, BIG[which], 0.02) + (BIG[which],)


def dup_max_case(nc=12):
    """128 x 128, two images (60 and 300 candidates), a third of the runner-up classes bit-identical to the maximum: the class must be
    the FIRST maximum.  (Kept out of the matrix above: torch's CPU max(1) returns another of the equal maxima, so the fp32 oracle cannot
    be compared on such rows.)"""
    return _case(f"dup_max nc {nc}", lambda at: Synth(128, 128, nc, (60, 300), 0.25, seed=60 + nc, dup_max=True, attempts=at), THRESHOLDS)


MASK_THR = (0.45, 0.7)


def mask_case(nc):
    """128 x 128, two images: the angle logit is +50 on every anchor (theta = 0.75 pi), above every class logit"""
    return _case(f"mask nc {nc}", lambda at: Synth(128, 128, nc, (60, 300), 0.25, seed=50 + nc, ang_logit=50.0, attempts=at), MASK_THR)


# Thin tiles (LetterBox(auto=True) turns a 10-px border crop into a 32 x 416 / 416 x 32 network input): 273 anchors in levels of 4 x 52,
# 2 x 26 and 1 x 13 with kCandCap's 256 | 257 hand-over INSIDE such an image and every anchor a candidate; 32 x 32: 21 anchors (16 + 4 + 1).
THIN_TILES = {(32, 416): (0, 1, 40, 256, 257, 273), (416, 32): (0, 1, 40, 256, 257, 273), (32, 32): (0, 1, 20, 21)}
THIN_CONF = (0.25, 0.001)


def thin_case(h, w, conf):
    """-> (Synth, [Case per image]) of the thin batch (h, w) at nc 12, decided at all five thresholds; tie blocks as in the matrix
    (two per image at 273 anchors, one at 21).  Objects are 0.12 .. 0.4 of the SHORT side: 4 .. 13 px boxes, many anchors per object."""
    ties = 2 if h * w > 32 * 32 else 1
    return _case(f"thin {h}x{w} conf {conf}", lambda at: Synth(h, w, 12, THIN_TILES[h, w], conf, seed=2000 + h + 3 * w, ties=ties, attempts=at), THRESHOLDS)


def all_cases():
    """every committed case, for make_postproc_attempts.py"""
    for (h, w) in THIN_TILES:
        for conf in THIN_CONF:
            thin_case(h, w, conf)
    for nc in NMS_NC:
        for conf in NMS_CONF:
            nms_matrix_case(nc, conf)
    for which in BIG:
        big_case(which)
    dup_max_case()
    for nc in (1, 4, 12, 15):
        mask_case(nc)


def results_rows(n=480, seed=3):
    """rows (x, y, w, h, conf, cls, theta) for k_results: angles on both sides of 0 and pi / 2 at distances 1e-6 .. 1e-2, random ones, and
    two rows ON a boundary (theta = 0 and theta = fp32(pi / 2)), whose swap is not decided: results64 must flag them"""
    g = torch.Generator().manual_seed(seed)
    det = torch.zeros((n, 7))
    det[:, 0:2] = torch.rand((n, 2), generator=g) * 416
    det[:, 2:4] = 5 + torch.rand((n, 2), generator=g) * 115
    det[:, 4] = 0.25 + 0.75 * torch.rand(n, generator=g)
    det[:, 5] = torch.randint(0, 12, (n,), generator=g).float()
    det[:, 6] = -math.pi / 4 + torch.rand(n, generator=g) * math.pi * 0.999
    k = 0
    for base in (0.0, math.pi / 2):
        for dist in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2):
            for sgn in (-1, 1):
                det[k, 6] = base + sgn * dist
                k += 1
    det[k, 6], det[k + 1, 6] = 0.0, HALF_PI32
    return det


def decode_inputs(h, w, nc, seed):
    """head [2, A, no] for the per-element decode test: DFL logits up to +-60, one-hot rows at bin 0 and bin 15, uniform rows, angle
    logits +-20 and 0, class logits up to +-30; padding columns zero (the test fills them)"""
    A = len(anchors(h, w)[1])
    g = torch.Generator().manual_seed(seed)
    hd = torch.zeros((2, A, no_of(nc)))
    body = torch.randn((2, A, 64 + nc + 1), generator=g)
    scale = torch.tensor([0.5, 2.0, 8.0, 30.0])[torch.randint(0, 4, (2, A, 1), generator=g)]
    body[..., :64] = (body[..., :64] * scale).clamp(-60, 60)
    body[..., 64:64 + nc] *= 4.0
    kind = torch.randint(0, 12, (2, A, 4), generator=g)  # per side: 0 one-hot bin 0, 1 one-hot bin 15, 2 uniform, 3 +-60 extremes
    sides = body[..., :64].reshape(2, A, 4, 16)
    onehot0 = torch.full((16,), -60.0); onehot0[0] = 60.0
    onehot15 = torch.full((16,), -60.0); onehot15[15] = 60.0
    sides[kind == 0] = onehot0
    sides[kind == 1] = onehot15
    sides[kind == 2] = 1.25
    ext = torch.where(torch.rand((2, A, 4, 16), generator=g) < 0.5, -60.0, 60.0)
    sides[kind == 3] = ext[kind == 3]
    body[..., :64] = sides.reshape(2, A, 64)
    ak = torch.randint(0, 8, (2, A), generator=g)
    ang = body[..., 64 + nc]
    ang[ak == 0], ang[ak == 1], ang[ak == 2] = 20.0, -20.0, 0.0
    body[0, :, 64] = torch.where(ak[0] == 3, 30.0, body[0, :, 64])
    body[1, :, 64 + nc - 1] = torch.where(ak[1] == 3, -30.0, body[1, :, 64 + nc - 1])
    hd[..., :64 + nc + 1] = body
    return hd


# ---------------------------------------------------------------------------------------------- result rows
def results64(det32, lb32=None):
    """construct_result on fp32 rows (x, y, w, h, conf, cls, theta) in fp64 -> (xywhr [n,5], corners [n,8], E_xywhr, E_corners, decided).
    The moduli are fp32(pi) and fp32(pi / 2), as `tensor % math.pi` evaluates on an fp32 tensor; fmod is exact, so theta carries one
    rounding (the sign fix-up r + b).  A row is decided when theta is further from every multiple of pi / 2 than 4 u |theta| + the
    difference of the fp32 moduli from their real values times the multiple.  Corners: cos / sin at L_ULP, w / 2 exact, products and the
    two additions one rounding each; with a letterbox row (gain, pad) one more for the subtraction and the division."""
    d = det32.double()
    x, y, w, h, t = d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 6]
    u = U
    kk = torch.round(t / (math.pi / 2))
    decided = (t - kk * (math.pi / 2)).abs() > 4 * u * t.abs() + (kk.abs() + 1) * abs(HALF_PI32 - math.pi / 2)
    swap = torch.remainder(t, PI32) >= HALF_PI32
    w_, h_ = torch.where(swap, h, w), torch.where(swap, w, h)
    tr = torch.remainder(t, HALF_PI32)
    Et = u * tr.abs()
    Ex, Ey, Ew, Eh = (torch.zeros_like(x) for _ in range(4))
    if lb32 is not None:
        l = lb32.double()
        gain, px, py = l[:, 0], l[:, 1], l[:, 2]
        Ex, Ey = (u * (x - px).abs() / gain + u * ((x - px) / gain).abs()), (u * (y - py).abs() / gain + u * ((y - py) / gain).abs())
        x, y, w_, h_ = (x - px) / gain, (y - py) / gain, w_ / gain, h_ / gain
        Ew, Eh = u * w_.abs(), u * h_.abs()
    c, s = torch.cos(tr), torch.sin(tr)
    Ec, Es = L_ULP * u * c.abs() + s.abs() * Et, L_ULP * u * s.abs() + c.abs() * Et
    v1x, v1y, v2x, v2y = w_ / 2 * c, w_ / 2 * s, -h_ / 2 * s, h_ / 2 * c
    E1x = Ew / 2 * c.abs() + w_ / 2 * Ec + u * v1x.abs()
    E1y = Ew / 2 * s.abs() + w_ / 2 * Es + u * v1y.abs()
    E2x = Eh / 2 * s.abs() + h_ / 2 * Es + u * v2x.abs()
    E2y = Eh / 2 * c.abs() + h_ / 2 * Ec + u * v2y.abs()
    pts, Ep = [], []
    for s1, s2 in ((1, 1), (1, -1), (-1, -1), (-1, 1)):
        for base, Eb, a, Ea, bb, Ebb in ((x, Ex, v1x, E1x, v2x, E2x), (y, Ey, v1y, E1y, v2y, E2y)):
            m = base + s1 * a
            pts.append(m + s2 * bb)
            Ep.append(Eb + Ea + Ebb + u * m.abs() + u * (m + s2 * bb).abs())
    xywhr = torch.stack([x, y, w_, h_, tr], -1)
    Exy = torch.stack([Ex, Ey, Ew, Eh, Et], -1) + 2.0 ** -149
    return xywhr, torch.stack(pts, -1), Exy, torch.stack(Ep, -1) + 2.0 ** -149, decided
