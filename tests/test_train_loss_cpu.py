"""CPU checks behind test_gpu_train_loss.py: the fp64 yardstick (oracle/loss.py) against formulations that share no code with it, and the
conditioning-floor helper (bounds.spread) on functions with known condition numbers."""
import math

import numpy as np
import torch

import train_loss_ref as R
from bounds import U, spread
from oracle import loss as ol


def _bhattacharyya(b1, b2):
    """matrix form: 1/8 dmu^T S^-1 dmu + 1/2 ln(det S / sqrt(det S1 det S2)), S = (S1 + S2) / 2, Si = R diag(w^2, h^2) / 12 R^T"""
    def cov(b):
        c, s = math.cos(b[4]), math.sin(b[4])
        Rm = np.array([[c, -s], [s, c]])
        return Rm @ np.diag([b[2] ** 2 / 12, b[3] ** 2 / 12]) @ Rm.T
    S1, S2 = cov(b1), cov(b2)
    S = (S1 + S2) / 2
    dm = np.array(b1[:2]) - np.array(b2[:2])
    return dm @ np.linalg.solve(S, dm) / 8 + 0.5 * math.log(np.linalg.det(S) / math.sqrt(np.linalg.det(S1) * np.linalg.det(S2)))


def test_probiou_matches_matrix_bhattacharyya():
    rng = np.random.default_rng(0)
    n = 300
    t = np.stack([rng.uniform(0, 400, n), rng.uniform(0, 400, n), rng.uniform(5, 100, n), rng.uniform(5, 100, n), rng.uniform(-3, 3, n)], 1)
    p = t + np.concatenate([rng.normal(0, 10, (n, 2)), rng.normal(0, 3, (n, 2)), rng.normal(0, 0.4, (n, 1))], 1)
    p[:, 2:4] = np.abs(p[:, 2:4]) + 1
    bd = np.array([_bhattacharyya(a, b) for a, b in zip(p, t)])
    keep = (bd > 1e-3) & (bd < 50)  # away from the eps and 100 clamps
    assert keep.sum() > 250
    hd = (1 - ol.probiou(torch.tensor(p), torch.tensor(t))).squeeze(-1).numpy()
    got = -np.log(1 + 1e-7 - hd ** 2)  # the oracle's bd, from hd = sqrt(1 - exp(-bd) + eps)
    err = np.abs(got - bd)[keep] / (1e-7 + 1e-6 * bd[keep])
    print("oracle bd vs matrix Bhattacharyya: max |d| / (1e-7 + 1e-6 bd)", err.max())
    assert err.max() <= 1  # the only difference: the restated formula's eps terms (eps / 2 inside the log, eps / D elsewhere)


def test_loss_oracles_gradcheck():
    g = torch.Generator().manual_seed(0)
    t = torch.tensor([[100.0, 100, 40, 20, 0.3], [50, 60, 30, 30, 1.0], [10, 10, 80, 8, -0.5]], dtype=torch.float64)
    p = (t + torch.randn(3, 5, generator=g, dtype=torch.float64) * torch.tensor([5, 5, 3, 3, 0.2], dtype=torch.float64)).requires_grad_(True)
    w = torch.tensor([0.5, 1.0, 0.25], dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda x: ol.probiou_loss(x, t, w, 2.0), (p,))
    x = torch.randn(5, 64, generator=g, dtype=torch.float64, requires_grad=True)
    tg = torch.tensor([[0.5, 3.2, 7.7, 14.2], [1.5, 2.25, 9.9, 0.1], [4.4, 5.6, 6.3, 13.3], [0.7, 8.8, 11.1, 12.6], [2.2, 3.3, 4.4, 5.5]], dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda z: ol.dfl_loss(z, tg, torch.ones(5, dtype=torch.float64), 3.0), (x,))
    y = torch.randn(2, 7, 3, generator=g, dtype=torch.float64, requires_grad=True)
    tt = torch.rand(2, 7, 3, generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda z: ol.bce_loss(z, tt, 1.7), (y,))


def _brute_assign(pds, pdb, anc, gtl, gtb, mgt, topk=10, alpha=0.5, beta=6.0, eps=1e-9):
    """the published RotatedTaskAlignedAssigner algorithm as a loop over (image, box, anchor), fp32 arithmetic via torch scalars"""
    bs, na, nc = pds.shape
    n_max = gtb.shape[1]
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    fg = torch.zeros(bs, na, dtype=torch.bool)
    ti = torch.zeros(bs, na, dtype=torch.long)
    ts = torch.zeros(bs, na, nc)
    for b in range(bs):
        ov = torch.zeros(n_max, na)
        me = torch.zeros(n_max, na)
        pos = torch.zeros(n_max, na, dtype=torch.bool)
        for g in range(n_max):
            if not mgt[b, g, 0]:
                continue
            corners = ol.xywhr2xyxyxyxy(gtb[b, g][None])[0]
            A, B, D = corners[0], corners[1], corners[3]
            ins = []
            for a in range(na):
                ab, ad, ap = B - A, D - A, anc[a] - A
                dab, dad = (ap * ab).sum(), (ap * ad).sum()
                inside = bool(dab >= 0) and bool(dab <= (ab * ab).sum()) and bool(dad >= 0) and bool(dad <= (ad * ad).sum())
                ins.append(inside)
                if inside:
                    ov[g, a] = ol.probiou(gtb[b, g][None], pdb[b, a][None]).squeeze().clamp(0)
                    me[g, a] = pds[b, a, int(gtl[b, g, 0])].pow(alpha) * ov[g, a].pow(beta)
            order = sorted(range(na), key=lambda a: (-float(me[g, a]), a))[:topk]  # largest metric, lowest anchor on ties
            for a in order:
                pos[g, a] = ins[a]
        for a in range(na):
            claims = [g for g in range(n_max) if pos[g, a]]
            if len(claims) > 1:
                best = max(range(n_max), key=lambda g: (float(ov[g, a]), -g))  # first maximum
                for g in range(n_max):
                    pos[g, a] = g == best
        for a in range(na):
            claims = [g for g in range(n_max) if pos[g, a]]
            if claims:
                fg[b, a] = True
                ti[b, a] = claims[0]
        for g in range(n_max):
            sel = pos[g]
            if not sel.any():
                continue
            pm, po = (me[g] * sel).max(), (ov[g] * sel).max()
            for a in torch.nonzero(sel).flatten().tolist():
                ts[b, a, int(gtl[b, g, 0])] = me[g, a] * po / (pm + f(eps))
    return fg, ti, ts


def test_assigner_oracle_matches_brute_force():
    rng = np.random.default_rng(3)
    pts = []
    for s, k in ((16, 13), (32, 7)):
        ys, xs = np.meshgrid(np.arange(k) + 0.5, np.arange(k) + 0.5, indexing="ij")
        pts.append(np.stack([xs.ravel() * s, ys.ravel() * s], 1))
    anc = torch.tensor(np.concatenate(pts), dtype=torch.float32)
    na = anc.shape[0]
    bs, n_max, nc = 3, 6, 5
    gtb = torch.tensor(np.stack([rng.uniform(30, 180, (bs, n_max)), rng.uniform(30, 180, (bs, n_max)), rng.uniform(20, 90, (bs, n_max)),
                                 rng.uniform(20, 90, (bs, n_max)), rng.uniform(-0.7, 2.3, (bs, n_max))], -1), dtype=torch.float32)
    gtb[0, 1] = gtb[0, 0]                                       # duplicate: the first wins
    gtb[1, 0] = torch.tensor([56.0, 56.0, 32.0, 32.0, 0.0])     # sides on stride-16 centres (40 and 72)
    gtl = torch.tensor(rng.integers(0, nc, (bs, n_max, 1)))
    mgt = torch.ones(bs, n_max, 1)
    mgt[2, 4:] = 0
    pdb = torch.cat([anc[None].expand(bs, -1, -1) + torch.tensor(rng.normal(0, 5, (bs, na, 2)), dtype=torch.float32),
                     torch.tensor(rng.uniform(20, 90, (bs, na, 2)), dtype=torch.float32), torch.tensor(rng.uniform(-0.7, 2.3, (bs, na, 1)), dtype=torch.float32)], -1)
    pds = torch.tensor(rng.uniform(0.01, 0.99, (bs, na, nc)), dtype=torch.float32)
    e_tl, e_tb, e_ts, e_fg, e_ti, _, _ = ol.rotated_tal_assign(pds, pdb, anc, gtl, gtb, mgt)
    fg, ti, ts = _brute_assign(pds, pdb, anc, gtl, gtb, mgt)
    assert int(fg.sum()) > 20
    assert torch.equal(fg, e_fg)
    assert torch.equal(ti[fg], e_ti[fg])
    assert torch.equal(e_tl[fg], gtl[torch.arange(bs)[:, None].expand(-1, na)[fg], ti[fg], 0])
    assert torch.equal(ts > 0, e_ts > 0) and torch.allclose(ts, e_ts.float(), rtol=1e-5, atol=0)  # pow on a vector and on a scalar differ in the last bit


def test_spread_on_known_condition_numbers():
    """relative spread / (16 u) of f at x is close to f's condition number |x f'(x) / f(x)| (inputs only; with 8 samples, within [0.3, 1])"""
    x = torch.tensor([1.5, 3.0, 100.0], dtype=torch.float64)
    for f, cond in ((lambda a, rnd: a * a, lambda a: 2.0), (lambda a, rnd: torch.sqrt(a), lambda a: 0.5), (lambda a, rnd: torch.exp(a), lambda a: a),
                    (lambda a, rnd: a - 1.4, lambda a: a / (a - 1.4))):
        v, s = spread(f, [x])
        r = (s / v.abs()) / (16 * U) / cond(x)
        assert bool((r <= 1.0 + 1e-6).all()) and bool((r >= 0.3).all()), r
    # an intermediate that cancels: (a + 1) - a with rnd on the sum has absolute spread ~ 2 u_mid (a + 1)
    big = torch.tensor([1e6], dtype=torch.float64)
    v, s = spread(lambda a, rnd: rnd(a + 1.0) - a, [big], rel=0.0, rel_mid=U)
    assert float(v) == 1.0 and 0.3e6 * U <= float(s) <= 1.0 * (1e6 + 1) * U


def test_optimizer_bounds_cover_fp32_torch():
    """the closed-form optimiser bounds hold for torch.optim's own fp32 step (the calibration the GPU test repeats)"""
    from bounds import _check
    g = torch.Generator().manual_seed(1)
    n = 4099
    p0 = torch.randn(n, generator=g) * 3
    for kind in ("sgd", "adamw"):
        ref = torch.nn.Parameter(p0.clone())
        opt = (torch.optim.SGD([ref], lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.1, foreach=False) if kind == "sgd"
               else torch.optim.AdamW([ref], lr=1e-2, weight_decay=0.1, foreach=False))
        for k in range(1, 6):
            p = ref.detach().clone()
            st = {key: v.clone() for key, v in opt.state.get(ref, {}).items() if torch.is_tensor(v)}
            gr = torch.randn(n, generator=g)
            gr[::5] = 0
            ref.grad = gr
            opt.step()
            if kind == "sgd":
                pn, bn, bp, bb = R.sgd_ref(p, gr, st.get("momentum_buffer"), 1e-2, 0.9, 0.1, True, k == 1)
                _check("sgd param", ref.detach(), pn, bp)
                _check("sgd buffer", opt.state[ref]["momentum_buffer"], bn, bb)
            else:
                m, v = st.get("exp_avg", torch.zeros(n)), st.get("exp_avg_sq", torch.zeros(n))
                pn, mn, vn, bp, bm, bv = R.adamw_ref(p, gr, m, v, k, 1e-2, (0.9, 0.999), 1e-8, 0.1)
                _check("adamw param", ref.detach(), pn, bp)
                _check("adamw exp_avg", opt.state[ref]["exp_avg"], mn, bm)
                _check("adamw exp_avg_sq", opt.state[ref]["exp_avg_sq"], vn, bv)


def test_dfl_bce_bounds_cover_fp32_torch():
    from bounds import _check
    g = torch.Generator().manual_seed(2)
    x = torch.randn(500, 64, generator=g) * 3
    x[0] = 80.0
    x[1, ::2] = -80.0
    t = torch.rand(500, 4, generator=g) * 17 - 1
    t[2] = torch.tensor([15.0, 14.99, 14.995, 0.0])
    w = torch.rand(500, generator=g)
    xr = x.clone().requires_grad_(True)
    ol.dfl_loss(xr, t, w, 7.0).backward()
    _, gr, _, bg = R.dfl_ref(x, t, w, float(np.float32(1) / np.float32(7.0)))
    _check("dfl grad, torch fp32", xr.grad, gr, bg)
    y = torch.cat([torch.tensor([90.0, -90.0, 17.0, -17.0, 0.0, 1e-30, -1e-30]), torch.randn(993, generator=g) * 5])
    tt = torch.where(torch.rand(1000, generator=g) < 0.3, torch.rand(1000, generator=g), torch.zeros(1000))
    yr = y.clone().requires_grad_(True)
    ol.bce_loss(yr, tt, 3.0).backward()
    _, gb, _, bb = R.bce_ref(y, tt, float(np.float32(1) / np.float32(3.0)))
    _check("bce grad, torch fp32", yr.grad, gb, bb)
