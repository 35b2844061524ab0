"""The loss, assigner and optimiser kernels (csrc/loss.hip, assigner.hip, optim.hip) per element against fp64 references of the same fp32
inputs (train_loss_ref.py: derivations of every bound).  Outputs go into Guarded buffers (NaN-filled, between guard bands).  Every check
prints its worst |err| / bound; where a bound is a conditioning floor, torch's own fp32 evaluation of the formula is checked against the
same bound in the same test (the calibration).  At the largest sizes the per-element checks cover every row within 2 of a 4096-block
boundary and a fixed sample of 1e5 rows; the scalar loss is always checked."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import train_loss_ref as R
from bounds import U, Guarded, _check, _same_thrice
from oracle import loss as ol

pytestmark = pytest.mark.gpu


def _ops():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    return ops, _lib


def _inv(tss):
    return float(np.float32(1.0) / np.float32(tss))  # the device's 1.0f / target_scores_sum


def _rows(n, seed=0):
    """every row within 2 of a 4096-block boundary and a fixed sample of 1e5 rows (all rows when n <= 1e5 + boundaries)"""
    if n <= 200000:
        return torch.arange(n)
    b = torch.arange(0, n + 4096, 4096)
    near = (b[:, None] + torch.arange(-2, 3)[None]).flatten()
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(0, n, (100000,), generator=g)
    return torch.unique(torch.cat([near[(near >= 0) & (near < n)], s, torch.tensor([0, n - 1])]))


# ---------------------------------------------------------------------------------------------- ProbIoU
def _random_pairs(rng, n):
    t = np.stack([rng.uniform(0, 416, n), rng.uniform(0, 416, n), rng.uniform(8, 120, n), rng.uniform(8, 120, n), rng.uniform(-np.pi / 4, 3 * np.pi / 4, n)], 1)
    p = t.copy()
    far = rng.uniform(size=n) < 0.3
    p[:, :2] += np.where(far[:, None], rng.normal(0, 60, (n, 2)), rng.normal(0, 4, (n, 2)))
    p[:, 2:4] *= rng.uniform(0.6, 1.6, (n, 2))
    p[:, 4] += rng.normal(0, 0.3, n)
    return p, t


def probiou_catalogue(seed=0):
    """-> (pred, target, weight) float32 and a dict kind -> row slice.  Kinds: random regime, identical, theta + pi twin, (theta + pi/2, h, w)
    twin, squares, aspect ratios 1..3000:1 at theta in {0, pi/4, pi/2, 0.3}, sizes 0.5..1500 px, bd around 100, weight 0."""
    rng = np.random.default_rng(seed)
    P, T, kinds = [], [], {}

    def add(kind, p, t):
        o = sum(len(x) for x in P)
        P.append(np.asarray(p, np.float64)); T.append(np.asarray(t, np.float64))
        kinds[kind] = slice(o, o + len(p))

    p, t = _random_pairs(rng, 600)
    add("random", p, t)
    t = _random_pairs(rng, 64)[1]
    add("identical", t, t)
    tw = t.copy(); tw[:, 4] += np.pi
    add("theta+pi", tw, t)
    ts = t.copy(); ts[:, 2], ts[:, 3] = t[:, 3], t[:, 2]; ts[:, 4] += np.pi / 2
    add("theta+pi/2 swapped", ts, t)
    sq = _random_pairs(rng, 64)[1]; sq[:, 3] = sq[:, 2]
    sp = sq.copy(); sp[:, :2] += rng.normal(0, 5, (64, 2)); sp[:, 3] = sp[:, 2] = sq[:, 2] * rng.uniform(0.8, 1.2, 64)
    add("square", sp, sq)
    th, tt = [], []
    for ar in (1, 10, 50, 200, 3000):
        for ang in (0.0, np.pi / 4, np.pi / 2, 0.3):
            for _ in range(6):
                w = 1500.0 if ar == 3000 else 20.0 * math.sqrt(ar)
                tt.append([200, 200, w, w / ar, ang])
                th.append([200 + rng.normal(0, 2), 200 + rng.normal(0, 2), w * rng.uniform(0.9, 1.1), w / ar * rng.uniform(0.9, 1.1), ang + rng.normal(0, 0.05)])
    add("aspect", th, tt)
    n = 128
    sz = np.exp(rng.uniform(np.log(0.5), np.log(1500), (n, 2)))
    t = np.stack([rng.uniform(0, 2000, n), rng.uniform(0, 2000, n), sz[:, 0], sz[:, 1], rng.uniform(-1, 2.5, n)], 1)
    p = t.copy(); p[:, :2] += rng.normal(0, 1, (n, 2)) * sz.mean(1, keepdims=True) * 0.3; p[:, 2:4] *= rng.uniform(0.7, 1.4, (n, 2))
    add("sizes", p, t)
    # w = h = 12 for both: A = B = 24, C = 0, bd = dx^2 / 96 -> bd = 100 at dx = sqrt(9600)
    d = math.sqrt(9600.0) * np.array([1 - 1e-2, 1 - 1e-4, 1 - 1e-6, 1.0, 1 + 1e-6, 1 + 1e-4, 1 + 1e-2])
    t = np.array([[100.0, 100.0, 12.0, 12.0, 0.0]] * len(d))
    p = t.copy(); p[:, 0] += d
    add("bd near 100", p, t)
    pred, target = (torch.tensor(np.concatenate(x), dtype=torch.float32) for x in (P, T))
    w = torch.tensor(rng.uniform(0.05, 1.0, pred.shape[0]), dtype=torch.float32)
    w[::17] = 0.0
    return pred, target, w, kinds


def _probiou_dev(ops, pred, target, w, tss):
    c = ops.ctx(torch.device("cuda"))
    n = pred.shape[0]
    loss, grad = Guarded((1,), torch.float32), Guarded((n, 5), torch.float32)
    pd, td = pred.cuda(), target.cuda()
    wd = w.cuda() if w is not None else None
    ops._call("obb_probiou_loss", c, ops._p(pd), ops._p(td), ops._p(wd), n, float(tss), ops._p(loss.out), ops._p(grad.out), ops._stream())
    return loss.get("probiou loss"), grad.get("probiou grad")


@pytest.mark.parametrize("tss", [1e-3, 1.0, 3e4])
def test_probiou_catalogue(tss):
    """The case catalogue, per pair: the per-pair loss (each pair in a call of its own: n = 1 returns it as the scalar), all 5 gradient
    components, and the scalar loss of the whole batch.  Identical pairs: loss at the clamp, gradient exactly 0."""
    ops, _ = _ops()
    pred, target, w, kinds = probiou_catalogue()
    inv = _inv(tss)
    l, g, braw, bl, bg = R.probiou_bounds(pred, target, w, inv)
    loss, grad = _probiou_dev(ops, pred, target, w, tss)
    print(f"tss {tss}: {pred.shape[0]} pairs, {int((~torch.isfinite(bg)).sum())} gradient elements without a finite conditioning floor")
    # calibration: torch's fp32 evaluation of the formula against the same bounds
    p32 = pred.clone().requires_grad_(True)
    L32 = ol.probiou_loss(p32, target, w, tss)
    L32.backward()
    ok = torch.isfinite(p32.grad).all(1)
    _check("calibration: torch fp32 grad", p32.grad[ok], g[ok], bg[ok])
    _check("calibration: torch fp32 loss_i", (1 - ol.probiou(pred, target)).squeeze(-1) * w, l, bl)
    for kind, s in kinds.items():
        _check(f"grad [{kind}]", grad[s], g[s], bg[s])
    Lref = float(l.sum()) * inv
    _check("scalar loss", loss, torch.tensor([Lref], dtype=torch.float64), torch.tensor([R.sum_bound(bl * inv, Lref, len(l))]))
    ident = kinds["identical"]
    assert bool((grad[ident] == 0).all()) and bool((p32.grad[ident] == 0).all()), "identical pairs: bd is below eps, the clamp blocks"
    # per-pair loss: n = 1 calls
    per = torch.stack([_probiou_dev(ops, pred[i:i + 1], target[i:i + 1], w[i:i + 1], 1.0)[0][0] for i in range(pred.shape[0])])
    _check("loss_i (n = 1 calls)", per, l, bl)
    assert bool((per[ident][w[ident] > 0] > 0).all())  # hd = sqrt(1 - exp(-eps) + eps) > 0 at the clamp
    # twins: the loss sits at the clamp, hd(eps) w, within its bound.  Their fp64 braw is ~0, but fp32 braw is rounding noise of the size
    # of eps itself, so which side of the gate fp32 takes is not determined: torch's fp32 passes the gradient on twin rows whose loss is
    # exactly at the clamp value.  The open gradient is 0 at a twin (bd has its minimum there), so the gradient bound of these rows is the
    # open gradient's rounding spread.
    for kind in ("theta+pi", "theta+pi/2 swapped"):
        s = kinds[kind]
        _check(f"loss_i at the clamp [{kind}]", per[s], l[s], bl[s])
        print(f"  {kind}: fp64 braw < eps on {int((braw[s] < R.PROBIOU_EPS).sum())} of {len(braw[s])}; max |grad| device "
              f"{float(grad[s].abs().max()):.3g}, torch fp32 {float(p32.grad[s].abs().max()):.3g}")
    # rows whose gradient bound reaches their largest gradient are checked only for finiteness: at the gates (identical, twins, bd = 100)
    # and thin boxes beyond 720:1 (kappa > 1 / (THIN u))
    unc = R.unchecked_rows(g, bg)
    print("  gradient rows checked only for finiteness, per kind:", {kd: int(unc[s].sum()) for kd, s in kinds.items()})
    assert not bool(unc[kinds["random"]].any()) and not bool(unc[kinds["square"]].any())
    assert int(unc[kinds["aspect"]].sum()) <= 24 and int(unc[kinds["sizes"]].sum()) <= 0.1 * len(unc[kinds["sizes"]])  # 24: the 3000:1 rows


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 4096 * 4096 + 1])
def test_probiou_sizes(n):
    """Block edges of the kernel (256) and of the sum (4096), and 4096^2 + 1 pairs: the three-level sum.  The pairs repeat a random block
    of 4099 (so the fp64 reference of every row, and the sum, come from that block); the rows near every 4096 boundary carry a loss."""
    ops, _ = _ops()
    rng = np.random.default_rng(n)
    m = min(n, 4099)
    p, t = _random_pairs(rng, m)
    pb, tb = torch.tensor(p, dtype=torch.float32), torch.tensor(t, dtype=torch.float32)
    wb = torch.tensor(rng.uniform(0.5, 1.0, m), dtype=torch.float32)
    reps = -(-n // m)
    pred, target, w = pb.repeat(reps, 1)[:n], tb.repeat(reps, 1)[:n], wb.repeat(reps)[:n]
    tss = float(w[:m].sum()) * n / m
    inv = _inv(tss)
    l, g, _, bl, bg = R.probiou_bounds(pb, tb, wb, inv)
    loss, grad = _probiou_dev(ops, pred, target, w, tss)
    rows = _rows(n)
    _check("grad", grad.cpu()[rows], g[rows % m], bg[rows % m])
    cnt = torch.bincount(torch.arange(n) % m, minlength=m).double() if n > m else torch.ones(m, dtype=torch.float64)
    Lref = float((l * cnt).sum()) * inv
    _check("scalar loss", loss, torch.tensor([Lref], dtype=torch.float64), torch.tensor([R.sum_bound(bl * cnt * inv, Lref, n)]))
    if n == 4097:  # the weightless form and the upstream gradient through loss.probiou_loss
        from oriented_object_detection_amd import loss as L
        l1, g1, _, bl1, bg1 = R.probiou_bounds(pb[:n], tb[:n], torch.ones(n), 1.0 / n)
        loss0, grad0 = _probiou_dev(ops, pred, target, None, float(n))
        _check("weightless grad", grad0, g1, bg1)
        _check("weightless loss", loss0, torch.tensor([float(l1.sum()) / n]), torch.tensor([R.sum_bound(bl1 / n, float(l1.sum()) / n, n)]))
        pd = pred.cuda().requires_grad_(True)
        (3.0 * L.probiou_loss(pd, target.cuda(), w.cuda(), tss)).backward()
        _check("3 x loss, autograd", pd.grad, 3.0 * g, 3.0 * bg + 3.0 * U * (3.0 * g).abs())


def test_probiou_same_after_growth():
    """bit-identical loss and gradient after a larger call grows WS_GEOM_A / WS_GEOM_B"""
    ops, _ = _ops()
    pred, target, w, _ = probiou_catalogue(1)
    big = torch.randn(3 * 4096 * 4096 // 2, 5).abs() + 1.0
    run = lambda: torch.cat([x.flatten() for x in _probiou_dev(ops, pred, target, w, 7.0)])
    _same_thrice("probiou", run, lambda: ops.probiou_loss(big.cuda(), big.cuda(), None, 1.0))


def test_probiou_weight_length_refused():
    ops, _ = _ops()
    p = torch.ones(10, 5).cuda()
    with pytest.raises(ValueError, match="weight"):
        ops.probiou_loss(p, p, torch.ones(9).cuda(), 1.0)
    with pytest.raises(ValueError, match="weight"):
        ops.probiou_loss(p, p, torch.ones(11).cuda(), 1.0)


# ---------------------------------------------------------------------------------------------- DFL
def _dfl_case(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 2.5, (n, 64)).astype(np.float32)
    t = rng.uniform(-0.5, 16.5, (n, 4)).astype(np.float32)
    special = np.array([0.0, 1.0, 7.0, 14.0, 15.0, 16.0, 14.99, np.nextafter(np.float32(14.99), np.float32(15)), 14.995, 14.9999, 14.98, -3.0, -1e-30,
                        np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(7), np.float32(0)), np.nextafter(np.float32(15), np.float32(0)), 20.0,
                        0.5], np.float32)
    k = min(n * 4, 4 * len(special))
    t.flat[:k] = np.resize(special, k)
    if n >= 8:
        x[0] = 80.0; x[1] = -80.0          # all equal
        x[2, ::16] = 80.0; x[3, 1::16] = -80.0; x[3, 5::16] = 80.0   # one-hot-like and +-80 spreads (exp overflows without the max shift)
        x[4] = rng.choice([-80.0, 80.0], 64)
        x[5, :16] = 0.0
    w = rng.uniform(0.05, 1.0, n).astype(np.float32)
    w[::7] = 0.0
    return torch.tensor(x), torch.tensor(t), torch.tensor(w)


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 300, 1025, 70001])
def test_dfl_per_element(n):
    """Targets: exact integers (wl = 1), 14.99 and inside (14.99, 15) and beyond (the clamp), negative, one ulp below an integer; logits
    +-80, all equal, one-hot-like; weight 0; 4 n not a multiple of 256."""
    ops, _lib = _ops()
    x, t, w = _dfl_case(n, n)
    tss = float(w.sum()) + 0.5
    inv = _inv(tss)
    l, g, bl, bg = R.dfl_ref(x, t, w, inv)
    c = ops.ctx(torch.device("cuda"))
    loss, grad = Guarded((1,), torch.float32), Guarded((n, 64), torch.float32)
    xd, td, wd = x.cuda(), t.cuda(), w.cuda()
    ops._call("obb_dfl_loss", c, ops._p(xd), ops._p(td), ops._p(wd), n, 16, float(tss), ops._p(loss.out), ops._p(grad.out), ops._stream())
    _check("grad", grad.get("dfl grad"), g, bg)
    Lref = float(l.sum())
    _check("scalar loss", loss.get("dfl loss"), torch.tensor([Lref], dtype=torch.float64), torch.tensor([R.sum_bound(bl, Lref, 4 * n)]))
    # calibration of the closed form: torch's fp32 evaluation of the oracle
    x32 = x.clone().requires_grad_(True)
    L32 = ol.dfl_loss(x32, t, w, tss)
    L32.backward()
    _check("calibration: torch fp32 grad", x32.grad, g, bg)
    _check("calibration: torch fp32 loss", L32.detach().reshape(1), torch.tensor([Lref], dtype=torch.float64), torch.tensor([R.sum_bound(bl, Lref, 4 * n)]))
    # weightless form
    l0, g0, bl0, bg0 = R.dfl_ref(x, t, None, _inv(float(n)))
    from oriented_object_detection_amd import loss as L
    xd2 = x.cuda().requires_grad_(True)
    L.dfl_loss(xd2, td, None, float(n)).backward()
    _check("weightless grad", xd2.grad, g0, bg0)


def test_dfl_alignment_refused():
    """a logits row that is not 16-byte aligned is refused with ObbHipError and the output is left untouched"""
    ops, _lib = _ops()
    n = 8
    x, t, w = _dfl_case(n, 3)
    buf = torch.zeros(n * 64 + 1, device="cuda")
    buf[1:].copy_(x.flatten().cuda())
    xv = buf[1:]
    loss, grad = Guarded((1,), torch.float32), Guarded((n, 64), torch.float32)
    c = ops.ctx(torch.device("cuda"))
    with pytest.raises(_lib.ObbHipError, match="aligned"):
        ops._call("obb_dfl_loss", c, ops._p(xv), ops._p(t.cuda()), ops._p(w.cuda()), n, 16, 1.0, ops._p(loss.out), ops._p(grad.out), ops._stream())
    torch.cuda.synchronize()
    assert loss.guards_intact() and grad.guards_intact()
    assert bool((loss.raw == 0xFF).all()) and bool((grad.raw == 0xFF).all()), "output written although the call was refused"


# ---------------------------------------------------------------------------------------------- BCE
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3549, 1), (3, 3549, 12), (2, 200, 80), (64, 3549, 80)])
def test_bce_per_element(shape):
    """x in {+-90, +-17, 0, +-1e-30} and random, t in {0, 1, fractional}; nc 1, 12, 80; 64 x 3549 x 80 > 4096^2 elements: three-level sum"""
    ops, _ = _ops()
    n = math.prod(shape)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(shape, generator=g) * 4 - 4
    tg = torch.where(torch.rand(shape, generator=g) < 0.05, torch.rand(shape, generator=g), torch.zeros(shape))
    xf, tf = x.view(-1), tg.view(-1)
    sp = torch.tensor([90.0, -90.0, 17.0, -17.0, 0.0, 1e-30, -1e-30])
    k = min(n, 3 * 7 * 50)
    xf[:k] = sp.repeat(150)[:k]
    tf[:k] = torch.tensor([0.0, 1.0, 0.3]).repeat_interleave(7).repeat(50)[:k]
    tf[k:k + 64] = 1.0
    tss = max(float(tg.sum()), 1.0)
    inv = _inv(tss)
    c = ops.ctx(torch.device("cuda"))
    loss, grad = Guarded((1,), torch.float32), Guarded(shape, torch.float32)
    xd, td = x.cuda(), tg.cuda()
    ops._call("obb_bce_loss", c, ops._p(xd), ops._p(td), n, float(tss), ops._p(loss.out), ops._p(grad.out), ops._stream())
    l, gr, bl, bg = R.bce_ref(x.view(-1), tf, inv)
    rows = _rows(n)
    _check("grad", grad.get("bce grad").view(-1).cpu()[rows], gr[rows], bg[rows])
    Lref = float(l.sum())
    _check("scalar loss", loss.get("bce loss"), torch.tensor([Lref], dtype=torch.float64), torch.tensor([R.sum_bound(bl, Lref, n)]))
    if n < 10 ** 6:
        x32 = x.clone().requires_grad_(True)
        L32 = ol.bce_loss(x32, tg, tss)
        L32.backward()
        _check("calibration: torch fp32 grad", x32.grad.view(-1), gr, bg)
        _check("calibration: torch fp32 loss", L32.detach().reshape(1), torch.tensor([Lref], dtype=torch.float64), torch.tensor([R.sum_bound(bl, Lref, n)]))


@pytest.mark.parametrize("n", [4095, 4096, 4097, 2 * 4096 + 1, 4096 * 4096, 4096 * 4096 + 1])
def test_sum_block_edges(n):
    """k_sum_f32's one-, two- and three-level paths, compared exactly.  BCE elements: x = 0, t = 0 (the device's fp32 log 2) everywhere but
    the last, x = -20, t = 1 (about 20).  The device's element values come from n = 1 calls (the scalar of one element with tss = 1 is that
    element).  Every block sum of these values is exact in double in any order, so the tree -- fp32(sum of each 4096-block), level by
    level, the last level times fp32(1 / tss) -- has one exact result, emulated here; dropping any block, or the last element, changes it."""
    ops, _ = _ops()
    x = torch.zeros(n)
    t = torch.zeros(n)
    x[-1], t[-1] = -20.0, 1.0
    loss, grad = ops.bce_loss(x.cuda(), t.cuda(), 1.0)
    v = float(ops.bce_loss(torch.zeros(1).cuda(), torch.zeros(1).cuda(), 1.0)[0][0])
    w = float(ops.bce_loss(torch.full((1,), -20.0).cuda(), torch.ones(1).cuda(), 1.0)[0][0])
    vals = np.full(n, v, np.float64)
    vals[-1] = w
    while True:  # k_sum_f32: fp32(double sum of each 4096-block x scale); scale = fp32(1 / tss) = 1 here
        nb = -(-len(vals) // 4096)
        part = np.zeros(nb * 4096)
        part[:len(vals)] = vals
        vals = part.reshape(nb, 4096).sum(1).astype(np.float32).astype(np.float64)
        if nb == 1:
            break
    print(f"n {n}: device {float(loss[0])!r}, emulated tree {float(vals[0])!r}, element log 2 -> {v!r}, last {w!r}")
    assert float(loss[0]) == float(vals[0])
    assert abs(float(grad[-1]) + 1) <= 4 * U  # sigmoid(-20) - 1
    assert float(grad[0]) == 0.5


# ---------------------------------------------------------------------------------------------- assigner
def _anchors(size):
    pts = []
    for s in (8, 16, 32):
        k = size // s
        ys, xs = np.meshgrid(np.arange(k) + 0.5, np.arange(k) + 0.5, indexing="ij")
        pts.append(np.stack([xs.ravel() * s, ys.ravel() * s], 1))
    return np.concatenate(pts).astype(np.float32)


def _preds_around(rng, anc, gtb, mgt, bs, nc):
    na = anc.shape[0]
    pdb = np.concatenate([anc[None] + rng.normal(0, 6, (bs, na, 2)), rng.uniform(10, 160, (bs, na, 2)), rng.uniform(-np.pi / 4, 3 * np.pi / 4, (bs, na, 1))], -1)
    for b in range(bs):
        for gi in np.nonzero(mgt[b, :, 0])[0]:
            near = np.argsort(np.abs(anc - gtb[b, gi, :2]).sum(1))[:25]
            pdb[b, near, :2] = gtb[b, gi, :2] + rng.normal(0, 3, (len(near), 2))
            pdb[b, near, 2:4] = gtb[b, gi, 2:4] * rng.uniform(0.8, 1.25, (len(near), 2))
            pdb[b, near, 4] = gtb[b, gi, 4] + rng.normal(0, 0.1, len(near))
    return pdb.astype(np.float32), rng.uniform(0.01, 0.99, (bs, na, nc)).astype(np.float32)


def assign_edge_case(nc=12, seed=0):
    """416 px, 3549 anchors.  Image 0: axis-aligned boxes at theta 0 and pi/2 whose sides lie on anchor centres of stride 8, 16 and 32;
    image 1: boxes with 0, 1 and fewer than topk in-box anchors, a duplicated box (the first must win), three boxes sharing anchors;
    image 2: random boxes; padded rows hold non-zero boxes and labels; labels 0 and nc - 1."""
    rng = np.random.default_rng(seed)
    anc = _anchors(416)
    bs, n_max = 3, 14
    gtb = rng.uniform(20, 300, (bs, n_max, 5)).astype(np.float32)  # padding: junk that must be ignored
    gtb[..., 4] = rng.uniform(-1, 2, (bs, n_max))
    gtl = rng.integers(0, nc, (bs, n_max, 1))
    mgt = np.zeros((bs, n_max, 1), np.float32)
    hp = np.float32(np.pi / 2)
    # sides on anchor centres: stride 8 centres at 4 + 8k, stride 16 at 8 + 16k, stride 32 at 16 + 32k
    box0 = [[100, 100, 64, 32, 0], [200, 108, 48, 16, hp],        # stride 8: edges at 4 + 8 k
            [72, 72, 64, 32, 0], [328, 72, 32, 64, hp],           # stride 16: edges at 8 + 16 k
            [112, 272, 128, 64, 0], [304, 336, 64, 128, hp],      # stride 32: edges at 16 + 32 k
            [52, 52, 8, 8, 0], [364, 364, 16, 32, hp]]
    gtb[0, :len(box0)] = box0
    mgt[0, :len(box0)] = 1
    box1 = [[101, 101, 2, 2, 0.3],  # no anchor inside
            [100, 100, 3, 3, 0.0],  # one anchor (100, 100) at stride 8: (100 - 4) / 8 = 12 -> centre 100
            [204, 204, 20, 12, 0.2], [204, 204, 20, 12, 0.2],  # duplicates
            [300, 300, 60, 40, 0.1], [305, 298, 50, 50, 0.5], [298, 303, 70, 30, -0.3],  # three boxes claiming the same anchors
            [60, 300, 24, 10, 0.7]]  # fewer than topk in-box anchors
    gtb[1, :len(box1)] = box1
    mgt[1, :len(box1)] = 1
    k = 9
    gtb[2, :k] = np.stack([rng.uniform(20, 396, k), rng.uniform(20, 396, k), rng.uniform(12, 150, k), rng.uniform(12, 150, k), rng.uniform(-np.pi / 4, 3 * np.pi / 4, k)], 1)
    mgt[2, :k] = 1
    gtl[0, 0, 0], gtl[0, 1, 0], gtl[1, 2, 0], gtl[1, 3, 0] = 0, nc - 1, nc - 1, nc - 1
    pdb, pds = _preds_around(rng, anc, gtb, mgt, bs, nc)
    return pds, pdb, anc, gtl, gtb, mgt


def assign_random_case(bs, n_max, nc, anc, seed):
    rng = np.random.default_rng(seed)
    lo, hi = float(anc.min()), float(anc.max())
    gtb = rng.uniform(lo, hi, (bs, n_max, 5)).astype(np.float32)
    gtl = rng.integers(0, nc, (bs, n_max, 1))
    mgt = np.zeros((bs, n_max, 1), np.float32)
    for b in range(bs):
        k = int(rng.integers(0, n_max + 1)) if b else n_max
        span = hi - lo
        gtb[b, :k] = np.stack([rng.uniform(lo, hi, k), rng.uniform(lo, hi, k), rng.uniform(0.03, 0.36, k) * span, rng.uniform(0.03, 0.36, k) * span,
                               rng.uniform(-np.pi / 4, 3 * np.pi / 4, k)], 1)
        mgt[b, :k] = 1
    pdb, pds = _preds_around(rng, anc, gtb, mgt, bs, nc)
    return pds, pdb, anc, gtl, gtb, mgt


def _inbox_margin(gt, anc):
    """fp64 (dab, nab - dab, dad, nad - dad) of the in-box test (oracle.select_candidates_in_gts) and their conditioning floor:
    FACTOR x spread with 16 u on the inputs and 2 u on the intermediates -> (min distance to a boundary, delta) per (box, anchor)"""
    def f(g, a, rnd):
        c, s = rnd(torch.cos(g[:, None, 4])), rnd(torch.sin(g[:, None, 4]))
        v1x, v1y = rnd(rnd(g[:, None, 2] / 2) * c), rnd(rnd(g[:, None, 2] / 2) * s)
        v2x, v2y = rnd(rnd(-g[:, None, 3] / 2) * s), rnd(rnd(g[:, None, 3] / 2) * c)
        ax, ay = rnd(rnd(g[:, None, 0] + v1x) + v2x), rnd(rnd(g[:, None, 1] + v1y) + v2y)
        bx, by = rnd(rnd(g[:, None, 0] + v1x) - v2x), rnd(rnd(g[:, None, 1] + v1y) - v2y)
        dx, dy = rnd(rnd(g[:, None, 0] - v1x) + v2x), rnd(rnd(g[:, None, 1] - v1y) + v2y)
        abx, aby, adx, ady = rnd(bx - ax), rnd(by - ay), rnd(dx - ax), rnd(dy - ay)
        px, py = rnd(a[None, :, 0] - ax), rnd(a[None, :, 1] - ay)
        dab, dad = rnd(rnd(px * abx) + rnd(py * aby)), rnd(rnd(px * adx) + rnd(py * ady))
        nab, nad = rnd(rnd(abx * abx) + rnd(aby * aby)), rnd(rnd(adx * adx) + rnd(ady * ady))
        return torch.stack([dab, nab - dab, dad, nad - dad], -1)

    from bounds import spread
    v, s = spread(f, [gt.double(), anc.double()], rel_mid=R.REL_MID)
    return v.abs().min(-1).values, (R.FACTOR * s + 8 * U * v.abs()).max(-1).values


def _overlap_spread(gt, pd):
    """fp64 overlap clamp(probiou(gt, pd), 0) and its conditioning floor (FACTOR x spread + 8 u overlap) for pairs [m, 5]"""
    from bounds import spread
    v, s = spread(lambda a, b, rnd: (1 - R.probiou_mc(a, b, rnd)[0]).clamp(0), [gt.double(), pd.double()], rel_mid=R.REL_MID)
    return v, R.FACTOR * s + 8 * U * v


def _oracle_claims(case, topk, alpha=0.5, beta=6.0):
    """the oracle's intermediates before select_highest_overlaps, by its own fp32 operations: (in-box mask, metric, positives before an
    anchor claimed by several boxes is resolved) [bs, n_max, na]"""
    pds, pdb, anc, gtl, gtb, mgt = (torch.as_tensor(x) for x in case)
    corners = ol.xywhr2xyxyxyxy(gtb)
    a_, b_, _, d_ = corners.split(1, dim=-2)
    ab, ad, ap = b_ - a_, d_ - a_, anc - a_
    dab, dad = (ap * ab).sum(-1), (ap * ad).sum(-1)
    inb = (dab >= 0) & (dab <= (ab * ab).sum(-1)) & (dad >= 0) & (dad <= (ad * ad).sum(-1)) & (mgt > 0)
    bs, na, nc = pds.shape
    n_max = gtb.shape[1]
    ov = torch.zeros(bs, n_max, na)
    ov[inb] = ol.probiou(gtb.unsqueeze(2).expand(-1, -1, na, -1)[inb], pdb.unsqueeze(1).expand(-1, n_max, -1, -1)[inb]).squeeze(-1).clamp_(0)
    sc = torch.zeros(bs, n_max, na)
    sc[inb] = pds[torch.arange(bs)[:, None], :, gtl[..., 0]][inb]
    metric = sc.pow(alpha) * ov.pow(beta)
    idx = torch.topk(metric, topk, dim=-1).indices
    cnt = torch.zeros(bs, n_max, na, dtype=torch.int32).scatter_add_(-1, idx, torch.ones_like(idx, dtype=torch.int32))
    return inb, metric, (cnt == 1) & inb


def _explain(b, a, got, exp, case, claims, topk, alpha=0.5, beta=6.0):
    """-> (kind, detail) of the near-tie behind a disagreement at (image b, anchor a), or None.  Only the boxes involved are asked: the
    device's box (where the device marks the anchor foreground) and the oracle's box (where the oracle does)."""
    pds, pdb, anc, gtl, gtb, mgt = case
    fg, ti, ts = got
    e_fg, e_ti, e_ts = exp
    inb, metric32, pos = claims
    boxes = sorted({int(x[b, a]) for x, f in ((ti, fg), (e_ti, e_fg)) if bool(f[b, a])})
    gts = torch.tensor(gtb[b], dtype=torch.float32)
    # in-box boundary: dab or dad within delta of 0 or of the squared side, for an involved box
    dist, delta = _inbox_margin(gts[boxes], torch.tensor(anc[a:a + 1]))
    for j, gi in enumerate(boxes):
        if float(dist[j, 0]) <= float(delta[j, 0]):
            return "in-box boundary", f"box {gi}: margin {float(dist[j, 0]):.3g} <= delta {float(delta[j, 0]):.3g}"
    # arg-max: both sides foreground on different boxes, the oracle saw several claimants, the two boxes' overlaps (both > 0) within delta
    if bool(fg[b, a]) and bool(e_fg[b, a]) and len(boxes) == 2 and int(pos[b, :, a].sum()) > 1:
        ov, dov = _overlap_spread(gts[boxes], torch.tensor(pdb[b, a]).expand(2, 5))
        if float(ov.min()) > 0 and abs(float(ov[0] - ov[1])) <= float(dov[0] + dov[1]):
            return "arg-max", f"boxes {boxes}: overlaps {float(ov[0]):.9g} / {float(ov[1]):.9g}"
    # topk boundary: the anchor is inside an involved box, and its metric is within delta of that box's topk-th / (topk+1)-th (> 0)
    row = torch.tensor(pdb[b])
    for gi in boxes:
        if not bool(inb[b, gi, a]):
            continue
        sc = torch.tensor(pds[b, :, int(gtl[b, gi, 0])]).double()
        o_all, do_all = _overlap_spread(gts[gi:gi + 1].expand(row.shape[0], 5), row)
        m_all = torch.where(inb[b, gi], sc.pow(alpha) * o_all.pow(beta), torch.zeros_like(o_all))
        dm_all = m_all * (beta * do_all / o_all.clamp_min(1e-300) + 4 * U)
        srt = torch.sort(m_all, descending=True)
        last = len(srt.indices) - 1
        for j in (topk - 1, topk):  # against the topk-th and the (topk+1)-th largest metric (itself: against its neighbour)
            kk = int(srt.indices[min(j, last)])
            if kk == a:
                kk = int(srt.indices[min(j + 1, last)]) if j == topk - 1 else int(srt.indices[j - 1])
            if kk != a and float(m_all[kk]) > 0 and abs(float(m_all[a] - m_all[kk])) <= float(dm_all[a] + dm_all[kk]):
                return "topk boundary", f"box {gi}: metric {float(m_all[a]):.9g} vs {float(m_all[kk]):.9g}"
    # topk tie at metric 0: the anchor is inside an involved box whose topk-th metric is 0 and so is the anchor's; the target score row
    # is 0 on both sides, so every loss term is the same
    for gi in boxes:
        kth = float(torch.sort(metric32[b, gi], descending=True).values[min(topk, metric32.shape[-1]) - 1])
        if bool(inb[b, gi, a]) and kth == 0.0 and float(metric32[b, gi, a]) == 0.0 and float(ts[b, a].abs().max()) == 0.0 \
                and float(e_ts[b, a].abs().max()) == 0.0:
            return "metric-0 topk tie", f"box {gi}"
    # the same below fp32's normal range: the box's topk-th metric (oracle) and the anchor's metric (fp64) are subnormal, where fp32 keeps
    # at most a few bits (overlap^6 of an overlap under ~1e-7); the target score rows on both sides are subnormal or 0
    for gi in boxes:
        kth = float(torch.sort(metric32[b, gi], descending=True).values[min(topk, metric32.shape[-1]) - 1])
        o, _ = _overlap_spread(gts[gi:gi + 1], torch.tensor(pdb[b, a:a + 1]))
        m64 = float(pds[b, a, int(gtl[b, gi, 0])]) ** alpha * float(o[0]) ** beta
        if bool(inb[b, gi, a]) and kth < R.F32_MIN and m64 < R.F32_MIN and float(ts[b, a].abs().max()) < R.F32_MIN \
                and float(e_ts[b, a].abs().max()) < R.F32_MIN:
            return "subnormal topk tie", f"box {gi}: metric {m64:.3g}, topk-th {kth:.3g}, target scores {float(ts[b, a].abs().max()):.3g} / {float(e_ts[b, a].abs().max()):.3g}"
    return None


def _assign_check(case, topk=10, what=""):
    ops, _ = _ops()
    pds, pdb, anc, gtl, gtb, mgt = case
    t = lambda a: torch.as_tensor(a)
    exp = ol.rotated_tal_assign(t(pds), t(pdb), t(anc), t(gtl), t(gtb), t(mgt), topk=topk)
    got = ops.rotated_tal_assign(t(pds).cuda(), t(pdb).cuda(), t(anc).cuda(), t(gtl).cuda(), t(gtb).cuda(), t(mgt).cuda(), topk=topk)
    torch.cuda.synchronize()
    tl, tb, ts, fg, ti = [g.cpu() for g in got]
    e_tl, e_tb, e_ts, e_fg, e_ti, e_metric, e_ov = exp
    diff = (fg != e_fg) | (fg & e_fg & (ti.long() != e_ti))
    claims = _oracle_claims(case, topk)
    kinds = {}
    for b, a in zip(*torch.nonzero(diff, as_tuple=True)):
        why = _explain(int(b), int(a), (fg, ti, ts), (e_fg, e_ti, e_ts), case, claims, topk)
        assert why is not None, (f"{what}: unexplained disagreement at image {int(b)} anchor {int(a)}: device fg {bool(fg[b, a])} gt {int(ti[b, a])}, "
                                 f"oracle fg {bool(e_fg[b, a])} gt {int(e_ti[b, a])}")
        kinds[why[0]] = kinds.get(why[0], 0) + 1
        print(f"  image {int(b)} anchor {int(a)}: {why[0]} ({why[1]})")
    print(f"{what}: {int(e_fg.sum())} foreground anchors, {int(diff.sum())} disagreements, named per kind: {kinds}")
    assert torch.equal(claims[2].any(1), e_fg), "the oracle's claims, recomputed, do not give its foreground"
    same = ~diff
    # everywhere else every discrete output is exact
    assert torch.equal(fg[same], e_fg[same])
    assert torch.equal(ti.long()[same], e_ti[same]), "target_gt_idx differs"
    assert torch.equal(tl.long()[same], e_tl[same]), "target_labels differ"
    assert torch.equal(tb[same], e_tb[same]), "target_bboxes differ"
    # target_scores per element: metric_a * max overlap / (max metric + eps) of the anchor's box; relative conditioning rho of each factor
    rows = same & e_fg
    if bool(rows.any()):
        bb, aa = torch.nonzero(rows, as_tuple=True)
        gi = e_ti[bb, aa]
        o, do = _overlap_spread(torch.tensor(gtb)[bb, gi], torch.tensor(pdb)[bb, aa])
        rho_o = do / o.clamp_min(1e-300)
        rho = 6 * rho_o + 4 * U  # metric = score^0.5 overlap^6
        # row maxima: the largest relative error over the row's positives
        key = bb * gtb.shape[1] + gi
        rmax = torch.zeros(gtb.shape[0] * gtb.shape[1], dtype=torch.float64).scatter_reduce(0, key, rho, "amax")
        tot = rho + 2 * rmax[key] + 4 * U
        lab = e_tl[bb, aa]
        ref = e_ts[bb, aa, lab].double()
        gotv = ts[bb, aa, lab].double()
        _check("target_scores (foreground, vs the fp32 oracle: 2 x the fp64 bound)", gotv, ref, 2 * tot * ref + 1e-30)
        other = ts[same].clone()
        other[e_fg[same]] = other[e_fg[same]].scatter(1, e_tl[same][e_fg[same]][:, None], 0.0)
        assert float(other.abs().max()) == 0.0, "target_scores: non-zero outside the assigned label"
    return exp, got


def test_assigner_edge_cases():
    for nc in (1, 12, 80):
        case = assign_edge_case(nc, seed=nc)
        exp, got = _assign_check(case, 10, f"edge cases nc {nc}")
        fg, ti = got[3].cpu(), got[4].cpu()
        e_fg, e_ti = exp[3], exp[4]
        # axis-aligned boxes with sides on anchor centres: the oracle puts the edge anchors inside (inclusive test)
        assert int(e_fg[0].sum()) > 0 and torch.equal(fg[0], e_fg[0]), "image 0: boxes on the anchor grid"
        # duplicates: the first of two identical boxes wins every anchor they share
        assert int((e_ti[1] == 2).sum()) > 0 and int((e_ti[1][e_fg[1]] == 3).sum()) == 0 and torch.equal(ti[1].long()[e_fg[1]], e_ti[1][e_fg[1]])
        # box 0 of image 1 has no anchor inside, box 1 exactly one
        assert int(((e_ti[1] == 0) & e_fg[1]).sum()) == 0 and int(((e_ti[1] == 1) & e_fg[1]).sum()) == 1


def test_assigner_inbox_exact_grid():
    """axis-aligned boxes on the anchor grid at all three strides: the device's in-box decisions equal the oracle's with no tolerance
    (theta 0: every product is exact; theta = fp32(pi/2): cos is -4.4e-8 on both sides, the build has no FMA contraction).  Each box is
    the only box of its own image and topk = the anchor count, so every in-box anchor is a positive: fg_mask is that box's in-box mask."""
    ops, _ = _ops()
    pds, pdb, anc, gtl, gtb, mgt = assign_edge_case(12, 0)
    na = anc.shape[0]
    k = 8
    case = (np.repeat(pds[:1], k, 0), np.repeat(pdb[:1], k, 0), anc, gtl[0, :k, None], gtb[0, :k, None], mgt[0, :k, None])
    t = lambda x: torch.as_tensor(x)
    inb = _oracle_claims(case, na)[0][:, 0]
    exp = ol.rotated_tal_assign(*(t(x) for x in case), topk=na)
    assert torch.equal(exp[3], inb)
    got = ops.rotated_tal_assign(*(t(x).cuda() for x in case), topk=na)
    print("in-box anchors per box:", inb.sum(1).tolist(), " device:", got[3].cpu().sum(1).tolist())
    assert torch.equal(got[3].cpu(), inb), "in-box decisions on the anchor grid differ"
    # and the edge anchors are really on the boundary: at theta 0 some anchors have dab or dad exactly 0 or equal to the squared side,
    # at fp32(pi / 2) within the rounding of cos (-4.4e-8 x the side)
    dist, delta = _inbox_margin(torch.tensor(gtb[0, :k]), torch.tensor(anc))
    at0 = torch.tensor(gtb[0, :k, 4] == 0)
    assert bool((dist[at0] == 0).any(1).all()) and bool((dist[~at0] <= delta[~at0]).any(1).all()) and na == 3549


@pytest.mark.parametrize("na", [1, 200, 3549, 8400, 10240])
def test_assigner_anchor_counts(na):
    rng = np.random.default_rng(na)
    if na == 3549:
        anc = _anchors(416)
    elif na == 8400:
        anc = _anchors(640)
    else:
        anc = rng.uniform(0, 416, (na, 2)).astype(np.float32)
    assert anc.shape[0] == na
    bs, n_max = (4, 9) if na <= 3549 else (2, 6)
    _assign_check(assign_random_case(bs, n_max, 12, anc, na), min(10, na), f"na {na}")  # (torch.topk needs topk <= na)


def test_assigner_refuses_10241_anchors():
    ops, _lib = _ops()
    anc = np.random.default_rng(0).uniform(0, 416, (10241, 2)).astype(np.float32)
    pds, pdb, anc, gtl, gtb, mgt = assign_random_case(1, 2, 12, anc, 0)
    t = lambda a: torch.as_tensor(a).cuda()
    with pytest.raises(_lib.ObbHipError, match="10240"):
        ops.rotated_tal_assign(t(pds), t(pdb), t(anc), t(gtl), t(gtb), t(mgt))


@pytest.mark.parametrize("topk,nc", [(1, 12), (10, 1), (13, 80)])
def test_assigner_topk(topk, nc):
    _assign_check(assign_random_case(3, 8, nc, _anchors(416), topk * 100 + nc), topk, f"topk {topk} nc {nc}")


def test_assigner_many_rows():
    """bs x n_max = 66 560 rows (> 65 535) over 200 anchors; most rows are padding filled with non-zero boxes and labels"""
    rng = np.random.default_rng(7)
    anc = rng.uniform(0, 416, (200, 2)).astype(np.float32)
    case = assign_random_case(128, 520, 12, anc, 11)
    pds, pdb, anc, gtl, gtb, mgt = case
    mgt[:, 6:] = 0  # at most 6 real boxes per image; the junk in the rows after them must be ignored
    _assign_check((pds, pdb, anc, gtl, gtb, mgt), 10, "128 x 520 rows")


# ---------------------------------------------------------------------------------------------- optimisers
OPT_CFGS = {
    "sgd_nesterov": dict(name="SGD", lr=1e-2, momentum=0.9, weight_decay=0.1, nesterov=True),
    "sgd_momentum": dict(name="SGD", lr=1e-2, momentum=0.9, weight_decay=0.1, nesterov=False),
    "sgd_plain": dict(name="SGD", lr=1e-2, momentum=0.0, weight_decay=0.1, nesterov=False),
    "adamw": dict(name="AdamW", lr=1e-2, momentum=0.9, weight_decay=0.1),
}


def _reference_cfgs():
    import oriented_object_detection_amd.train as TR
    out = {}
    for key, kw in (("ref_sgd", dict(name="SGD")), ("ref_auto_adamw", dict(name="auto"))):
        c = TR.optimizer_config(12, 100, lr0=0.003, weight_decay=0.001, **kw)
        out[key] = dict(name=c["name"], lr=c["lr"], momentum=c["momentum"], weight_decay=c["weight_decay"], nesterov=True)
    assert out["ref_auto_adamw"]["name"] == "AdamW" and out["ref_sgd"]["lr"] == 0.003
    return out


def _grad_seq(n, steps, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(steps):
        v = torch.randn(n, generator=g) * (0.1 + k % 3)
        v[::5] = 0.0                                                   # exactly 0 (eps and the decay alone move these)
        v[1::7] = torch.randn(len(v[1::7]), generator=g) * 1e-7        # tiny: eps is a large part of the denominator
        out.append(v)
    return out


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1027, 100003])
@pytest.mark.parametrize("cfg", list(OPT_CFGS) + ["ref_sgd", "ref_auto_adamw"])
def test_optimizer_per_element(n, cfg):
    """20 steps of torch.optim (foreach=False, fp32, CPU).  Before every step the device state (Guarded buffers: the momentum buffer is
    NaN-filled before the first step, which must not read it) is set to torch's; after it the parameters and every state buffer are
    compared per element with the fp64 step from that state (train_loss_ref.sgd_ref / adamw_ref), and so are torch's own.  In the
    decisive configurations the decay, the momentum, Nesterov, the bias corrections and eps each move the result by >= 100 x the bound."""
    ops, _ = _ops()
    kw = OPT_CFGS[cfg] if cfg in OPT_CFGS else _reference_cfgs()[cfg]
    gs = _grad_seq(n, 20, n)
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(n + 1)) * 3
    ref = torch.nn.Parameter(p0.clone())
    adam = kw["name"] == "AdamW"
    if adam:
        topt = torch.optim.AdamW([ref], lr=kw["lr"], betas=(kw["momentum"], 0.999), eps=1e-8, weight_decay=kw["weight_decay"], foreach=False)
    else:
        topt = torch.optim.SGD([ref], lr=kw["lr"], momentum=kw["momentum"], nesterov=kw["nesterov"], weight_decay=kw["weight_decay"], foreach=False)
    P, G = Guarded((n,), torch.float32), Guarded((n,), torch.float32)
    S = [Guarded((n,), torch.float32) for _ in range(2 if adam else 1)]
    decisive = cfg in OPT_CFGS
    moved = {}
    for k in range(1, 21):
        p = ref.detach().clone()
        st = topt.state.get(ref, {})
        P.out.copy_(p)
        G.out.copy_(gs[k - 1])
        if adam:
            m = st["exp_avg"].clone() if st else torch.zeros(n)
            v = st["exp_avg_sq"].clone() if st else torch.zeros(n)
            S[0].out.copy_(m); S[1].out.copy_(v)
            ops.adamw_step(P.out, G.out, S[0].out, S[1].out, k, kw["lr"], (kw["momentum"], 0.999), 1e-8, kw["weight_decay"])
            pn, mn, vn, bp, bm, bv = R.adamw_ref(p, gs[k - 1], m, v, k, kw["lr"], (kw["momentum"], 0.999), 1e-8, kw["weight_decay"])
            if decisive:
                for term, alt in (("decay", dict(no_decay=True)), ("eps", dict(eps_inside=True))):
                    q = R.adamw_ref(p, gs[k - 1], m, v, k, kw["lr"], (kw["momentum"], 0.999), 1e-8, kw["weight_decay"], **alt)[0]
                    moved[term] = max(moved.get(term, 0.0), float(((q - pn).abs() / bp).max()))
                if k <= 2:  # the bias corrections: without them step_size = lr, sqrt_bc2 = 1
                    q = R.adamw_ref(p, gs[k - 1], m, v, 10 ** 6, kw["lr"], (kw["momentum"], 0.999), 1e-8, kw["weight_decay"])[0]
                    moved[f"bias corrections, step {k}"] = float(((q - pn).abs() / bp).max())
        else:
            first = k == 1
            b = None if first or not kw["momentum"] else st["momentum_buffer"].clone()
            if b is not None:
                S[0].out.copy_(b)
            ops.sgd_step(P.out, G.out, S[0].out, kw["lr"], kw["momentum"], kw["weight_decay"], kw["nesterov"], first)
            pn, bn, bp, bb = R.sgd_ref(p, gs[k - 1], b, kw["lr"], kw["momentum"], kw["weight_decay"], kw["nesterov"], first)
            if decisive:
                q = R.sgd_ref(p, gs[k - 1], b, kw["lr"], kw["momentum"], 0.0, kw["nesterov"], first)[0]
                moved["decay"] = max(moved.get("decay", 0.0), float(((q - pn).abs() / bp).max()))
                if kw["momentum"] and not first:
                    q = R.sgd_ref(p, gs[k - 1], b, kw["lr"], kw["momentum"], kw["weight_decay"], not kw["nesterov"], first)[0]
                    moved["nesterov"] = max(moved.get("nesterov", 0.0), float(((q - pn).abs() / bp).max()))
                    q = R.sgd_ref(p, gs[k - 1], b * 0, kw["lr"], kw["momentum"], kw["weight_decay"], kw["nesterov"], first)[0]
                    moved["momentum"] = max(moved.get("momentum", 0.0), float(((q - pn).abs() / bp).max()))
        ref.grad = gs[k - 1].clone()
        topt.step()
        tst = topt.state[ref]
        quiet = k not in (1, 2, 20)
        ctx = contextlib.redirect_stdout(io.StringIO()) if quiet else contextlib.nullcontext()  # print steps 1, 2 and 20
        if not quiet:
            print(f"{cfg} n {n} step {k}:")
        with ctx:
            _check("param", P.get("param"), pn, bp)
            _check("calibration: torch param", ref.detach(), pn, bp)
            if adam:
                _check("exp_avg", S[0].get("exp_avg"), mn, bm)
                _check("exp_avg_sq", S[1].get("exp_avg_sq"), vn, bv)
                _check("calibration: torch exp_avg", tst["exp_avg"], mn, bm)
                _check("calibration: torch exp_avg_sq", tst["exp_avg_sq"], vn, bv)
            elif kw["momentum"]:
                _check("momentum_buffer", S[0].get("momentum_buffer"), bn, bb)
                _check("calibration: torch momentum_buffer", tst["momentum_buffer"], bn, bb)
            else:
                assert bool((S[0].raw == 0xFF).all()), "momentum 0: the buffer must not be touched"
    if decisive and n >= 1023:
        print(f"{cfg}: max effect of each term / bound: " + ", ".join(f"{t} {v:.3g}" for t, v in moved.items()))
        for t, v in moved.items():
            assert v >= 100, f"{cfg}: the {t} term moves the result by only {v:.3g} x the bound"
