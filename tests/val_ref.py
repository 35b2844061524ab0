"""CPU side of the validation tests (train.Validator, ops.val_match, metrics.ap_per_class) -- not the product, nothing here touches the GPU.
Written from the rules (Ultralytics 8.3.x restated from recall, UNPINNED), not from the product code:

  probiou(a, b, dtype)            batch_probiou's covariance form (eps 1e-7) for every pair of two box lists, evaluated in `dtype` throughout
  match(...)                      the validator's matching rule in fp64: best class-equal unmasked ground truth per detection (ties to the lower
                                  index), claim iff IoU >= threshold, the lowest claiming index per (ground truth, threshold) is the true positive
  compute_ap / ap_per_class       the 101-point AP, plain Python loops in float
  match_cases(seed)               the data of the matching tests, shared by the CPU margin test and the GPU test
  pair_ious(case, dtype)          the ProbIoU of every candidate pair (live detection, unmasked class-equal ground truth) of a case"""
import numpy as np

THR = np.linspace(0.5, 0.95, 10).astype(np.float32)
SEED = 3  # chosen so that test_validate_cpu's margin assertions hold (they are asserted, not assumed)


def _cov(b, dt):
    w, h, t = b[:, 2].astype(dt), b[:, 3].astype(dt), b[:, 4].astype(dt)
    a, bb, c, s = w * w / dt(12), h * h / dt(12), np.cos(t), np.sin(t)
    return a * c * c + bb * s * s, a * s * s + bb * c * c, (a - bb) * c * s


def probiou(g, p, dtype=np.float64):
    """g [n,5], p [m,5] (x, y, w, h, theta) -> [n, m]"""
    dt = np.dtype(dtype).type
    g, p = np.asarray(g).astype(dt), np.asarray(p).astype(dt)
    eps = dt(1e-7)
    a1, b1, c1 = (v[:, None] for v in _cov(g, dt))
    a2, b2, c2 = (v[None, :] for v in _cov(p, dt))
    x1, y1, x2, y2 = g[:, 0][:, None], g[:, 1][:, None], p[:, 0][None, :], p[:, 1][None, :]
    with np.errstate(all="ignore"):
        den = (a1 + a2) * (b1 + b2) - (c1 + c2) * (c1 + c2) + eps
        t1 = (((a1 + a2) * (y1 - y2) * (y1 - y2) + (b1 + b2) * (x1 - x2) * (x1 - x2)) / den) * dt(0.25)
        t2 = (((c1 + c2) * (x2 - x1) * (y1 - y2)) / den) * dt(0.5)
        d1, d2 = np.maximum(a1 * b1 - c1 * c1, dt(0)), np.maximum(a2 * b2 - c2 * c2, dt(0))
        t3 = np.log(((a1 + a2) * (b1 + b2) - (c1 + c2) * (c1 + c2)) / (dt(4) * np.sqrt(d1 * d2) + eps) + eps) * dt(0.5)
        bd = np.clip(t1 + t2 + t3, eps, dt(100))
        return (dt(1) - np.sqrt(dt(1) - np.exp(-bd) + eps)).astype(dt)


def _valid_det(row, nc):
    return bool(np.isfinite(row[[0, 1, 2, 3, 6]]).all()) and bool(0 <= row[5] < nc)


def candidates(det_b, count_b, gl_b, gb_b, mk_b, nc):
    """-> [(d, [g, ...])]: per live, valid detection the unmasked, valid, class-equal ground truths"""
    out = []
    for d in range(min(max(int(count_b), 0), len(det_b))):
        if not _valid_det(det_b[d], nc):
            continue
        c = int(det_b[d, 5])
        gs = [g for g in range(len(gl_b)) if mk_b[g] and 0 <= gl_b[g] < nc and gl_b[g] == c and np.isfinite(gb_b[g]).all()]
        out.append((d, gs))
    return out


def match(det, count, gl, gb, mk, nc, thr=THR):
    """-> (tp uint16 [B,max_det], best_iou float64 [B,max_det], best_gt int32 [B,max_det]) in fp64"""
    B, M = det.shape[:2]
    tp, bi, bg = np.zeros((B, M), np.uint16), np.zeros((B, M)), np.full((B, M), -1, np.int32)
    thr = np.asarray(thr, np.float64)  # (the float32 thresholds' exact values)
    for b in range(B):
        for d, gs in candidates(det[b], count[b], gl[b], gb[b], mk[b], nc):
            if not gs:
                continue
            iou = probiou(gb[b][gs], det[b][d:d + 1, [0, 1, 2, 3, 6]])[:, 0]
            best = -1.0
            for g, v in zip(gs, iou):
                if v > best:
                    best, bg[b, d] = v, g
            bi[b, d] = best
        for i, t in enumerate(thr):
            taken = set()
            for d in range(M):  # ascending index = descending confidence: the first claim wins
                g = bg[b, d]
                if g >= 0 and bi[b, d] >= t and g not in taken:
                    taken.add(g)
                    tp[b, d] |= 1 << i
    return tp, bi, bg


def pair_ious(case, dtype):
    """every candidate pair's ProbIoU in `dtype` -> [(b, d, [g...], iou [len])]"""
    det, count, gl, gb, mk, nc = case
    out = []
    for b in range(det.shape[0]):
        for d, gs in candidates(det[b], count[b], gl[b], gb[b], mk[b], nc):
            if gs:
                out.append((b, d, gs, probiou(gb[b][gs], det[b][d:d + 1, [0, 1, 2, 3, 6]], dtype)[:, 0].astype(np.float64)))
    return out


# ---------------------------------------------------------------------------------------------------------------- AP
def compute_ap(recall, precision):
    mrec = [0.0] + [float(r) for r in recall] + [1.0]
    mpre = [1.0] + [float(p) for p in precision] + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    xs = list(np.linspace(0, 1, 101))
    ys = []
    for x in xs:  # linear interpolation over the non-decreasing recall points; at a repeated point the LAST of the repeats counts (np.interp's rule)
        if x >= mrec[-1]:
            ys.append(mpre[-1]); continue
        j = int(np.searchsorted(np.asarray(mrec), x, side="right"))
        x0, x1, y0, y1 = mrec[j - 1], mrec[j], mpre[j - 1], mpre[j]
        ys.append(y0 + (y1 - y0) * (x - x0) / (x1 - x0))
    return sum((ys[i] + ys[i + 1]) / 2.0 * (xs[i + 1] - xs[i]) for i in range(100))


def ap_per_class(tp, conf, pred_cls, target_cls, nc):
    tp, conf, pred_cls, target_cls = np.asarray(tp, bool), np.asarray(conf, np.float64), np.asarray(pred_cls), np.asarray(target_cls)
    order = sorted(range(len(conf)), key=lambda i: -conf[i])  # Python's sort is stable
    classes = sorted({int(c) for c in target_cls})
    T = tp.shape[1]
    ap = np.zeros((len(classes), T))
    for ci, c in enumerate(classes):
        n_gt = int((target_cls == c).sum())
        idx = [i for i in order if int(pred_cls[i]) == c]
        for j in range(T):
            t = f = 0
            rec, pre = [], []
            for i in idx:
                t, f = t + int(tp[i, j]), f + int(not tp[i, j])
                rec.append(t / (n_gt + 1e-16)); pre.append(t / (t + f))
            ap[ci, j] = compute_ap(rec, pre) if idx else 0.0
    map50 = float(ap[:, 0].mean()) if ap.size else 0.0
    mean = float(ap.mean()) if ap.size else 0.0
    return {"ap": ap, "map50": map50, "map": mean, "fitness": 0.1 * map50 + 0.9 * mean}


# ---------------------------------------------------------------------------------------------------------------- matching cases
def _jitter(rng, g, t):
    """a copy of box g moved by t x its extent in a random direction, sides within 5 %, angle within 0.05 rad: IoU ~ 1 - sqrt(1 - exp(-1.5 t^2))"""
    a = rng.uniform(0, 2 * np.pi)
    c, s = np.cos(g[4]), np.sin(g[4])
    du, dv = t * g[2] * np.cos(a), t * g[3] * np.sin(a)
    return np.array([g[0] + du * c - dv * s, g[1] + du * s + dv * c, g[2] * rng.uniform(0.95, 1.05), g[3] * rng.uniform(0.95, 1.05), g[4] + rng.uniform(-0.05, 0.05)])


def match_cases(seed=SEED, B=4, max_det=300, n_cap=64, nc=3):
    """-> (det fp32 [B,max_det,7], count int32 [B], gt_labels int32 [B,n_cap], gt_bboxes fp32 [B,n_cap,5], mask_gt bool [B,n_cap], nc).
    image 0: 300 detections on 64 ground truths (a grid, far apart; every detection a jittered copy of a same-class ground truth, IoU 0.3 .. 1: many
             share one); image 1: the hand-built 7 on 5 (below); image 2: one detection, no ground truth; image 3: one ground truth, no detection.
    Rows at or past the count and masked rows: NaN boxes, classes far outside [0, nc)."""
    rng = np.random.RandomState(seed)
    det = np.full((B, max_det, 7), np.nan, np.float32)
    det[:, :, 5] = 1e9
    gl, gb, mk = np.full((B, n_cap), -7, np.int32), np.full((B, n_cap, 5), np.nan, np.float32), np.zeros((B, n_cap), bool)
    gl[:, 1::2] = 10 ** 6
    count = np.array([300, 7, 1, 0], np.int32)[:B]
    n_gt = [64, 5, 0, 1][:B]

    def put_det(b, rows):
        conf = np.sort(rng.uniform(0.01, 0.99, len(rows)))[::-1]
        for d, (box, c) in enumerate(rows):
            det[b, d] = (box[0], box[1], box[2], box[3], conf[d], c, box[4])

    # image 0
    g0 = []
    for i in range(n_gt[0]):
        g0.append((np.array([50 + 100 * (i % 8) + rng.uniform(-5, 5), 50 + 100 * (i // 8) + rng.uniform(-5, 5), rng.uniform(20, 60), rng.uniform(20, 60),
                             rng.uniform(0, np.pi / 2)]), int(rng.randint(0, nc))))
    rows = []
    for d in range(count[0]):
        box, c = g0[rng.randint(0, len(g0))]
        rows.append((_jitter(rng, box, rng.uniform(0.0, 0.67)), c))
    put_det(0, rows)
    # image 1: g0 and g1 overlap (same class 0); g2 is the only ground truth of class 1... and g3, g4 class 2
    a = np.array([200.0, 200.0, 60.0, 40.0, 0.3])
    g1 = [(a, 0), (_jitter(rng, a, 0.35), 0), (np.array([500.0, 200.0, 50.0, 50.0, 1.0]), 1), (np.array([200.0, 500.0, 40.0, 70.0, 0.7]), 2),
          (np.array([500.0, 500.0, 30.0, 30.0, 0.1]), 2)]
    toward = a + 0.12 * (g1[1][0] - a)
    rows = [(_jitter(rng, a, 0.05), 0),            # d0 takes g0
            (toward, 0),                           # d1: best g0 (taken by d0), second g1 above 0.5: stays unmatched
            (_jitter(rng, g1[3][0], 0.1), 1),      # d2: a high-IoU box on g3 with the WRONG class (1): its only candidate is the far g2
            (_jitter(rng, g1[3][0], 0.2), 2),      # d3 and d4: two detections on g3
            (_jitter(rng, g1[3][0], 0.3), 2),
            (_jitter(rng, g1[4][0], 0.6), 2),      # d5: IoU ~ 0.35 with g4: under every threshold
            (_jitter(rng, g1[2][0], 0.15), 1)]     # d6 on g2
    put_det(1, rows)
    if B > 2:
        put_det(2, [(np.array([100.0, 100.0, 30.0, 20.0, 0.5]), 1)])
    for b, gs in enumerate([g0, g1, [], [(np.array([300.0, 300.0, 40.0, 40.0, 0.2]), 2)]][:B]):
        for i, (box, c) in enumerate(gs):
            gl[b, i], gb[b, i], mk[b, i] = c, box, True
    return det, count, gl, gb, mk, nc


def tiny_case():
    """n_cap = 1, max_det = 1: one detection on its ground truth"""
    det = np.array([[[10.0, 12.0, 8.0, 6.0, 0.9, 0.0, 0.4]]], np.float32)
    return det, np.array([1], np.int32), np.array([[0]], np.int32), np.array([[[10.5, 12.0, 8.0, 6.0, 0.4]]], np.float32), np.array([[True]]), 1


def band(cases):
    """4 x the largest |fp32 - fp64| of any candidate pair's ProbIoU (both evaluated here, on the CPU) -> (band, fp64 pair list per case)"""
    worst, p64s = 0.0, []
    for case in cases:
        p32, p64 = pair_ious(case, np.float32), pair_ious(case, np.float64)
        for (_, _, _, a), (_, _, _, b) in zip(p32, p64):
            worst = max(worst, float(np.abs(a - b).max()))
        p64s.append(p64)
    return 4.0 * worst, p64s
