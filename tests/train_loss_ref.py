"""fp64 references and per-element error bounds for the loss, assigner and optimiser kernels (csrc/loss.hip, assigner.hip, optim.hip).
Used by test_gpu_train_loss.py (against the device) and test_train_loss_cpu.py (calibration against torch's own fp32 evaluation of
the same formulas, and the oracle against formulations that share no code with it).  u = 2^-24.

ProbIoU and the assigner's overlap use the conditioning floor of bounds.spread: probiou_mc restates oracle/loss.py's probiou operation by
operation, with a rounding hook after every fp32 operation; the bound of an element is FACTOR x (its spread over K = 8 evaluations with
every input perturbed by up to 16 u and every intermediate by up to 2 u, one fp32 rounding plus one ulp of libm) + an absolute floor.
The other bounds are closed forms; each function states its derivation."""
import numpy as np
import torch

from bounds import U, spread

FACTOR = 8.0      # times the spread (calibrated: torch's fp32 evaluation passes with margin, see test_train_loss_cpu.py)
REL_MID = 2 * U   # perturbation of the intermediates
THIN = 32.0       # thin-box term of the ProbIoU gradient bound (probiou_bounds)
PROBIOU_EPS = 1e-7
F32_MIN = 2.0 ** -126


def f32(x):
    """the value the device sees: x rounded to fp32, as fp64"""
    return torch.as_tensor(x).float().double()


# ---------------------------------------------------------------------------------------------- ProbIoU
def probiou_mc(b1, b2, rnd=lambda t: t, eps=PROBIOU_EPS, gate=True):
    """oracle.loss.probiou (fp64) with rnd() after every operation that rounds in fp32 -> (1 - iou = hd, braw = t1 + t2 + t3).
    gate=False: bd = braw without the clamp to [eps, 100] (the gradient the clamp passes or blocks)."""
    def cov(b):
        a = rnd(rnd(b[:, 2] * b[:, 2]) / 12)
        bb = rnd(rnd(b[:, 3] * b[:, 3]) / 12)
        c, s = rnd(torch.cos(b[:, 4])), rnd(torch.sin(b[:, 4]))
        c2, s2 = rnd(c * c), rnd(s * s)
        return rnd(rnd(a * c2) + rnd(bb * s2)), rnd(rnd(a * s2) + rnd(bb * c2)), rnd(rnd(rnd(a - bb) * c) * s)

    a1, b1_, c1 = cov(b1)
    a2, b2_, c2 = cov(b2)
    A, B, C = rnd(a1 + a2), rnd(b1_ + b2_), rnd(c1 + c2)
    dx, dy = rnd(b1[:, 0] - b2[:, 0]), rnd(b1[:, 1] - b2[:, 1])
    D = rnd(rnd(A * B) - rnd(C * C))
    den = rnd(D + eps)
    t1 = rnd(rnd(rnd(rnd(A * rnd(dy * dy)) + rnd(B * rnd(dx * dx))) / den) * 0.25)
    t2 = rnd(rnd(rnd(rnd(C * -dx) * dy) / den) * 0.5)
    d1 = rnd(rnd(a1 * b1_) - rnd(c1 * c1)).clamp(0)
    d2 = rnd(rnd(a2 * b2_) - rnd(c2 * c2)).clamp(0)
    g = rnd(rnd(4 * rnd(rnd(d1 * d2).sqrt())) + eps)
    t3 = rnd(rnd(torch.log(rnd(rnd(D / g) + eps))) * 0.5)
    braw = rnd(rnd(t1 + t2) + t3)
    bd = braw.clamp(eps, 100.0) if gate else braw
    hd = rnd(rnd(rnd(1.0 - rnd(torch.exp(-bd))) + eps).sqrt())
    return hd, braw


def probiou_elem(pred, target, weight, inv_tss, rnd=lambda t: t, gate=True):
    """per pair: (loss_i = hd_i w_i, d (sum_j loss_j inv_tss) / d pred_i [n,5], braw_i) in fp64 by autograd through probiou_mc"""
    p = pred.detach().clone().requires_grad_(True)
    hd, braw = probiou_mc(p, target, rnd, gate=gate)
    l = hd * weight
    (g,) = torch.autograd.grad(l.sum() * inv_tss, p)
    return l.detach(), g, braw.detach()


def probiou_bounds(pred, target, weight, inv_tss, k=8, seed=0):
    """-> (loss_i, grad_i, braw_i, bound on loss_i, bound on grad_i), fp64, from fp32 inputs.
    bound = FACTOR * spread + floor; floor(loss_i) = 8 u loss_i (the rounding of hd * w), floor(grad) = 8 u |grad| + 1e-30 + the thin-box
    term below.
    The clamp of bd to [eps, 100] passes the gradient inside and blocks it outside; where braw lies within its own error (FACTOR * spread
    + 8 u |braw|) of either end, fp32 may take the other side: the gradient bound there adds the open-gate gradient (and its spread).
    A perturbed evaluation that is not finite (sqrt / log at a clamp) makes that element's spread infinite: no bound there but finiteness."""
    pred, target, weight = pred.double(), target.double(), weight.double()
    inv = float(inv_tss)

    def f(p, t, w, rnd):
        l, g, b = probiou_elem(p, t, w, inv, rnd)
        _, go, _ = probiou_elem(p, t, w, inv, rnd, gate=False)
        return l, g, b, go

    (l, g, braw, go), sp = spread(f, [pred, target, weight], k=k, seed=seed, rel_mid=REL_MID)
    sl, sg, sb, sgo = (torch.nan_to_num(x, nan=float("inf")) for x in sp)
    db = FACTOR * sb + 8 * U * braw.abs()
    near = ((braw - PROBIOU_EPS).abs() <= db) | ((braw - 100.0).abs() <= db)
    # the gradient's chain cancels where a box is thin: d1 = A1 B1 - C1^2 = a b loses the factor kappa = max(a, b) / min(a, b) = (w / h)^2
    # of its accuracy, and the partial derivatives through it cancel against each other by as much, beyond what the spread sees:
    # + THIN kappa u max_j |grad_ij| per row.  THIN is fitted: over the catalogue and 2000 further pairs of 0.5..1500 px sides, torch's fp32
    # gradient needed at most 16.6 (a 421 x 4 px pair, kappa 1.1e4, its theta gradient 2.3 % off) and 0 on every row with kappa < 1e4.
    # The term reaches the row's largest gradient at kappa = 1 / (THIN u) = 5.2e5 (aspect 720:1): such rows are only checked for
    # finiteness, and unchecked_rows() counts them.
    wh = torch.cat([pred[:, 2:4], target[:, 2:4]], 1).abs()
    kappa = (wh[:, [0, 2]].maximum(wh[:, [1, 3]]) / wh[:, [0, 2]].minimum(wh[:, [1, 3]]).clamp_min(1e-30)).pow(2).amax(1)
    bg = (FACTOR * sg + 8 * U * g.abs() + 1e-30 + torch.where(near[:, None], go.abs() + FACTOR * sgo, torch.zeros_like(go))
          + (THIN * kappa * U * g.abs().amax(1))[:, None])
    return l, g, braw, FACTOR * sl + 8 * U * l.abs(), bg


def unchecked_rows(grad_ref, bound):
    """rows whose every gradient bound reaches the row's largest |gradient| (or is not finite): checked only for finiteness"""
    return (bound >= grad_ref.abs().amax(1, keepdim=True)).all(1) & (grad_ref.abs().amax(1) > 0) | ~torch.isfinite(bound).all(1)


def sum_bound(elem_bound, ref_sum, n):
    """a scalar loss of n fp32 elements >= 0 through k_sum_f32's tree: each level sums 4096-blocks in double (any order: n 2^-53 |L| in
    all) and rounds every block sum to fp32 (u |L| per level; the last level's single block is the result), the result is scaled by the
    fp32 inv_tss (u |L|).  -> sum of the element bounds (already scaled by inv_tss) + (levels + 1) u |L| + n 2^-53 |L|."""
    levels = 1 if n <= 4096 else (2 if n <= 4096 * 4096 else 3)
    return float(elem_bound.sum()) + ((levels + 1) * U + n * 2.0 ** -53) * abs(ref_sum) + 1e-30


# ---------------------------------------------------------------------------------------------- DFL
DFL_HI = float(np.float32(15.0) - np.float32(0.01))  # the clamp's upper end as fp32 evaluates 15 - 0.01


def dfl_ref(logits, target, weight, inv_tss):
    """fp64 from fp32 inputs (the upper clamp at fp32(15 - 0.01), the constant the device and torch's fp32 use) and the closed-form bounds.
    -> (loss_i per (box, side) * inv_tss, grad [n, 64], bound loss_i, bound grad).
    Per (box, side), fp32 with roundings u (libm exp / log: 2 u):
      e_k = exp(x_k - m): rel. error eps_k = u |x_k - m| + 2 u      (the subtraction rounds, then exp)
      se = sum of 16 positive terms: rel. error eps_se = 16 u + max_k eps_k;  p_k = e_k (1 / se): eps_k + eps_se + 2 u
      wl = tr - t, wr = 1 - wl: absolute u each;  gs = (w / 4) (1 / tss): 2 u relative
      grad_k = (p_k - [k = tl] wl - [k = tr] wr) gs:
        |err| <= gs (p_k (eps_k + eps_se + 2 u) + 2 u (wl + wr) + 2 u |p_k - w_k|) + 2 u |grad_k| + 2 gs F32_MIN (exp underflow)
      loss_i = ((lse - x_l) wl + (lse - x_r) wr) w / 4, lse = m + log se:
        |err lse| <= u |lse| + 2 u |log se| + eps_se;  |err| <= w/4 ((wl + wr)(err lse + u) + 3 u ((lse - x_l) wl + (lse - x_r) wr))"""
    x = logits.double().reshape(-1, 16)
    t = target.double().reshape(-1).clamp(0, DFL_HI)
    w = (weight.double() if weight is not None else torch.ones(target.shape[0], dtype=torch.float64)).repeat_interleave(4)
    tl = t.long()
    tr = tl + 1
    wl = tr - t
    wr = 1 - wl
    m = x.max(1, keepdim=True).values
    e = torch.exp(x - m)
    se = e.sum(1, keepdim=True)
    p = e / se
    lse = (m + torch.log(se)).squeeze(1)
    xl = x.gather(1, tl[:, None]).squeeze(1)
    xr = x.gather(1, tr.clamp(max=15)[:, None]).squeeze(1)
    gs = w * 0.25 * inv_tss
    oh = torch.zeros_like(x)
    oh.scatter_(1, tl[:, None], wl[:, None])
    oh.scatter_add_(1, tr.clamp(max=15)[:, None], torch.where(tr <= 15, wr, torch.zeros_like(wr))[:, None])
    grad = (p - oh) * gs[:, None]
    eps_k = U * (x - m).abs() + 2 * U
    eps_se = 16 * U + eps_k.max(1, keepdim=True).values
    bg = gs[:, None] * (p * (eps_k + eps_se + 2 * U) + 2 * U * (wl + wr)[:, None] + 2 * U * (p - oh).abs()) + 2 * U * grad.abs() + 2 * gs[:, None] * F32_MIN
    loss = ((lse - xl) * wl + (lse - xr) * wr) * w * 0.25
    e_lse = U * lse.abs() + 2 * U * torch.log(se).abs().squeeze(1) + eps_se.squeeze(1)
    bl = w * 0.25 * ((wl + wr) * (e_lse + U) + 3 * U * ((lse - xl).abs() * wl + (lse - xr).abs() * wr)) + U * loss.abs()
    return loss * inv_tss, grad.reshape(logits.shape), bl * inv_tss, bg.reshape(logits.shape)


# ---------------------------------------------------------------------------------------------- BCE
def bce_ref(logits, target, inv_tss):
    """fp64 from fp32 inputs and closed-form bounds -> (loss_i * inv_tss, grad_i, bound loss_i, bound grad_i).
    fp32: ea = exp(-|x|) (2 u); l = max(x, 0) - x t + log1p(ea): the product, two sums and log1p (2 u) ->
      |err l| <= 4 u (max(x, 0) + |x t| + log1p(ea)) + 2 u ea
    sig = 1 / (1 + ea) or ea / (1 + ea): 4 u relative; (sig - t) inv_tss: u |sig - t| for the difference, 2 u for inv_tss and the product ->
      |err grad| <= (4 u sig + 3 u |sig - t|) inv_tss"""
    x, t = logits.double(), target.double()
    ea = torch.exp(-x.abs())
    l1 = torch.log1p(ea)
    loss = x.clamp(min=0) - x * t + l1
    sig = torch.sigmoid(x)
    grad = (sig - t) * inv_tss
    bl = 4 * U * (x.clamp(min=0) + (x * t).abs() + l1) + 2 * U * ea
    bg = (4 * U * sig + 3 * U * (sig - t).abs() + 2 * F32_MIN) * inv_tss  # + exp underflow below FLT_MIN
    return loss * inv_tss, grad, bl * inv_tss, bg


# ---------------------------------------------------------------------------------------------- optimisers
def sgd_ref(p, g, buf, lr, mu, wd, nesterov, first):
    """one torch.optim.SGD step (dampening 0) in fp64 from the fp32 state and fp32 constants -> (p', buf', bound p', bound buf').
    Magnitudes D = |g| + wd |p|, M = mu |buf| + D, N = D + mu M (nesterov) or M; each fp32 operation rounds by u of its result:
      d = g + wd p: 2 u D;  buf' = mu buf + d: 4 u M;  d' = d + mu buf': 6 u N;  p' = p - lr d': 2 u |p| + 8 u lr N"""
    lr, mu, wd = (float(np.float32(v)) for v in (lr, mu, wd))
    p, g = p.double(), g.double()
    d = g + wd * p
    D = g.abs() + wd * p.abs()
    if mu != 0:
        b = d if first else mu * buf.double() + d
        M = D if first else mu * buf.double().abs() + D
        dd = d + mu * b if nesterov else b
        N = D + mu * M if nesterov else M
    else:
        b, M, dd, N = None, None, d, D
    pn = p - lr * dd
    bp = 2 * U * p.abs() + 8 * U * lr * N + 1e-45
    bb = 4 * U * M + 1e-45 if b is not None else None
    return pn, b, bp, bb


def adamw_consts(lr, betas, step):
    """the constants the device receives: torch's bias corrections in double from the (double) betas, rounded to fp32"""
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return float(np.float32(lr / bc1)), float(np.float32(bc2 ** 0.5))


def adamw_ref(p, g, m, v, step, lr, betas, eps, wd, eps_inside=False, no_decay=False):
    """one torch.optim.AdamW step in fp64 from the fp32 state (1 - beta exact, from the Python betas) -> (p', m', v', bounds of each).
    fp32 roundings (u each):
      p1 = p (1 - lr wd): 3 u |p|
      m' = m + (g - m)(1 - b1): 4 u Mm, Mm = |m| + (1 - b1)(|g| + |m|)
      v' = b2 v + (1 - b2) g g (all terms >= 0): 4 u v'
      denom = sqrt(v') / sqrt_bc2 + eps: 6 u denom (sqrt halves v's 4 u; the constant, the division and the sum add u each)
      p' = p1 - step_size m' / denom: 3 u |p| + 2 u |p'| + step_size (4 u Mm + 10 u |m'|) / denom
    plus the rounding of the constant 1 - beta_i to fp32, c_i = u (1 - b_i), which moves m' by c1 |g - m|, v' by c2 g^2 and p' by
    step_size (that of m' + |m'| c2 g^2 / (2 sqrt(v') sqrt_bc2 denom)) / denom.  (Taking 1 - fp32(beta) instead, 1.0f - 0.999f, is
    1.3e-5 off 0.001; bias corrections from fp32 betas put 6.5e-6 on every update: both fail these bounds.)
    `eps_inside` / `no_decay` give the update with eps under the square root / without the decoupled decay (how much those terms move
    the result)."""
    b1, b2 = betas
    lr32, eps32, wd32 = (float(np.float32(c)) for c in (lr, eps, wd))
    c1, c2 = U * (1 - b1), U * (1 - b2)
    ss, sbc2 = adamw_consts(lr, betas, step)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    p1 = p if no_decay else p * (1 - lr32 * wd32)
    mn = m + (g - m) * (1 - b1)
    vn = v * b2 + (1 - b2) * g * g
    denom = (vn + eps32).sqrt() / sbc2 if eps_inside else vn.sqrt() / sbc2 + eps32
    pn = p1 - ss * (mn / denom)
    Mm = m.abs() + (1 - b1) * (g.abs() + m.abs())
    bm = 4 * U * Mm + c1 * (g - m).abs() + 1e-45
    bv = 4 * U * vn + c2 * g * g + 1e-45
    dden = c2 * g * g / (2 * vn.sqrt().clamp_min(1e-300) * sbc2)
    bp = (3 * U * p.abs() + 2 * U * pn.abs() + ss * (4 * U * Mm + 10 * U * mn.abs() + c1 * (g - m).abs()) / denom
          + ss * mn.abs() * dden / (denom * denom) + 1e-45)
    return pn, mn, vn, bp, bm, bv
