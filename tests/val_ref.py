"""CPU side of the validation tests (train.Validator, ops.val_match, metrics.ap_per_class) -- not the product, nothing here touches the GPU.
Written from the rules (Ultralytics 8.3.x restated from recall, UNPINNED), not from the product code:

  probiou(a, b, dtype)            batch_probiou's covariance form (eps 1e-7) for every pair of two box lists, evaluated in `dtype` throughout
  match(...)                      the validator's matching rule in fp64: best class-equal unmasked ground truth per detection (ties to the lower
                                  index), claim iff IoU >= threshold, the lowest claiming index per (ground truth, threshold) is the true positive
  compute_ap / ap_per_class       the 101-point AP, plain Python loops in float
  match_cases(seed)               the data of the matching tests, shared by the CPU margin test and the GPU test
  edge_cases()                    more of them at the kernel's edges: sizes up to the declared limits, 1 and 16 thresholds, forced ties, invalid live
                                  rows, counts outside [0, max_det]; all_cases() / all_band(): old and new together and their band
  pair_ious(case, dtype)          the ProbIoU of every candidate pair (live detection, unmasked class-equal ground truth) of a case"""
import functools

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
    gl_b = np.asarray(gl_b)
    ok_g = np.asarray(mk_b, bool) & (gl_b >= 0) & (gl_b < nc) & np.isfinite(np.asarray(gb_b)).all(1)  # (once per image: the rule is per ground truth)
    for d in range(min(max(int(count_b), 0), len(det_b))):
        if not _valid_det(det_b[d], nc):
            continue
        c = int(det_b[d, 5])
        out.append((d, np.flatnonzero(ok_g & (gl_b == c)).tolist()))
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
    det, count, gl, gb, mk, nc = case[:6]
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


# ---------------------------------------------------------------------------------------------------------------- matching cases at the edges
def _blank(B, max_det, n_cap):
    """every row dead: NaN boxes, classes far outside [0, nc), nothing unmasked"""
    det = np.full((B, max_det, 7), np.nan, np.float32)
    det[:, :, 5] = 1e9
    gl, gb, mk = np.full((B, n_cap), -7, np.int32), np.full((B, n_cap, 5), np.nan, np.float32), np.zeros((B, n_cap), bool)
    gl[:, 1::2] = 10 ** 6
    return det, gl, gb, mk


def _grid(rng, n, nc, cols):
    """n ground truths far apart: 100 px pitch, sides 20 .. 60 px"""
    return [(np.array([50 + 100 * (i % cols) + rng.uniform(-5, 5), 50 + 100 * (i // cols) + rng.uniform(-5, 5), rng.uniform(20, 60), rng.uniform(20, 60),
                       rng.uniform(0, np.pi / 2)]), int(rng.randint(0, nc))) for i in range(n)]


def _put_det(rng, det, b, rows):
    conf = np.sort(rng.uniform(0.01, 0.99, len(rows)))[::-1]
    for d, (box, c) in enumerate(rows):
        det[b, d] = (box[0], box[1], box[2], box[3], conf[d], c, box[4])


def _put_gt(gl, gb, mk, b, gs):
    for i, (box, c) in enumerate(gs):
        gl[b, i], gb[b, i], mk[b, i] = c, box, True


def _on(rng, gs, n, tmax, pick=None):
    """n detections, each a jittered copy of one of `gs` (of those listed in `pick`) with its class"""
    pick = list(range(len(gs))) if pick is None else pick
    return [(_jitter(rng, gs[g][0], rng.uniform(0.0, tmax)), gs[g][1]) for g in (pick[rng.randint(0, len(pick))] for _ in range(n))]


def size_case(n_cap, max_det, thr, seed, tmax=0.67, nc=3):
    """B = 2.  Image 0: every one of the n_cap rows an unmasked ground truth on a grid, max_det live detections (a lane of the kernel owns
    ceil(max_det / 256) of them); image 1: 7 ground truths, max_det // 2 detections, the rest dead rows."""
    rng = np.random.RandomState(seed)
    det, gl, gb, mk = _blank(2, max_det, n_cap)
    g0, g1 = _grid(rng, n_cap, nc, 32), _grid(rng, min(7, n_cap), nc, 4)
    rows = _on(rng, g0, max_det, tmax)
    rows[-1] = (_jitter(rng, g0[-1][0], 0.1), g0[-1][1])  # the last detection row on the last ground-truth row
    _put_det(rng, det, 0, rows)
    _put_det(rng, det, 1, _on(rng, g1, max_det // 2, tmax))
    _put_gt(gl, gb, mk, 0, g0)
    _put_gt(gl, gb, mk, 1, g1)
    return det, np.array([max_det, max_det // 2], np.int32), gl, gb, mk, nc, np.asarray(thr, np.float32), f"size-{n_cap}x{max_det}-thr{len(thr)}"


TIE_GT = (3, 9)              # two ground truths with identical rows and class
TIE_DETS = (40, 90, 140, 190)  # detections placed on them
TIE_NEXT = (20, 30)         # detections 20 and 21 identical, on ground truth 30 alone
TIE_LANE = (5, 261, 31)      # detections 5 and 261 identical (one lane of the kernel, successive passes), on ground truth 31 alone


def ties_case(seed):
    """B = 1, 300 detection rows (270 live) on 40 ground truths.  The ties are exact by construction: equal rows give equal fp32 results."""
    rng = np.random.RandomState(seed)
    det, gl, gb, mk = _blank(1, 300, 64)
    gs = _grid(rng, 40, 3, 8)
    gs[TIE_GT[1]] = (gs[TIE_GT[0]][0].copy(), gs[TIE_GT[0]][1])
    free = [g for g in range(40) if g not in (TIE_NEXT[1], TIE_LANE[2])]
    rows = _on(rng, gs, 270, 0.67, free)
    for k, d in enumerate(TIE_DETS):  # at least these sit on the twin ground truths
        rows[d] = (_jitter(rng, gs[TIE_GT[k % 2]][0], 0.05 * (k + 1)), gs[TIE_GT[0]][1])
    rows[TIE_NEXT[0]] = rows[TIE_NEXT[0] + 1] = (_jitter(rng, gs[TIE_NEXT[1]][0], 0.1), gs[TIE_NEXT[1]][1])
    rows[TIE_LANE[0]] = rows[TIE_LANE[1]] = (_jitter(rng, gs[TIE_LANE[2]][0], 0.1), gs[TIE_LANE[2]][1])
    _put_det(rng, det, 0, rows)
    _put_gt(gl, gb, mk, 0, gs)
    return det, np.array([270], np.int32), gl, gb, mk, 3, THR, "ties"


BAD_DET = {3: "nan-x", 10: "inf-w", 17: "class--1", 24: "class-nc", 31: "class-nan", 38: "class-1e9", 45: "nan-theta"}
BAD_GT = {20: "nan-x", 21: "label--1", 22: "label-nc"}


def invalid_case(seed, bad=True):
    """B = 1, 64 detection rows (50 live) on 20 ground truths of classes 0..2, nc = 4.  bad: the live rows BAD_DET and the unmasked rows BAD_GT are
    invalid, each sitting exactly on a valid ground truth (the class -1 / nc detections on the label -1 / nc ground truths).  not bad: the same data
    with those detections in class 3, which no ground truth has, and those ground truths masked out: every row's result must be the same."""
    rng = np.random.RandomState(seed)
    nc = 4
    det, gl, gb, mk = _blank(1, 64, 32)
    gs = _grid(rng, 20, 3, 5)
    rows = _on(rng, gs, 50, 0.67)
    for k, d in enumerate(BAD_DET):
        rows[d] = (gs[k][0].copy(), gs[k][1])
    rows[17], rows[24] = (gs[1][0].copy(), gs[1][1]), (gs[2][0].copy(), gs[2][1])
    _put_det(rng, det, 0, rows)
    _put_gt(gl, gb, mk, 0, gs + [(gs[0][0].copy(), gs[0][1]), (gs[1][0].copy(), -1), (gs[2][0].copy(), nc)])
    gb[0, 20, 0] = np.nan
    if bad:
        det[0, 3, 0], det[0, 10, 2], det[0, 45, 6] = np.nan, np.inf, np.nan
        det[0, 17, 5], det[0, 24, 5], det[0, 31, 5], det[0, 38, 5] = -1.0, nc, np.nan, 1e9
    else:
        det[0, list(BAD_DET), 5] = 3.0
        mk[0, list(BAD_GT)] = False
    return det, np.array([50], np.int32), gl, gb, mk, nc, THR, "invalid-rows" if bad else "invalid-rows-clean"


def counts_case(seed, clamped=False):
    """B = 2, every row of both images valid: count = max_det + 7 behaves as max_det, count = -4 as 0 (clamped: the same data with those counts)"""
    rng = np.random.RandomState(seed)
    det, gl, gb, mk = _blank(2, 40, 16)
    for b in range(2):
        gs = _grid(rng, 12, 3, 4)
        _put_det(rng, det, b, _on(rng, gs, 40, 0.67))
        _put_gt(gl, gb, mk, b, gs)
    return det, np.array([40, 0] if clamped else [47, -4], np.int32), gl, gb, mk, 3, THR, "counts-clamped" if clamped else "counts"


THR16 = np.linspace(0.2, 0.95, 16).astype(np.float32)
EDGE_SEEDS = {"size0": 21, "size1": 12, "size2": 13, "size3": 51, "ties": 15, "invalid": 16, "counts": 17}  # re-seeded until test_validate_cpu's margins hold


@functools.lru_cache(maxsize=None)
def edge_cases():
    """[(det, count, gt_labels, gt_bboxes, mask_gt, nc, thr, name)]: the matching cases at the kernel's launch and domain edges (the first six as
    `match_cases()` returns them).  Built once per process; nobody writes into them."""
    S = EDGE_SEEDS
    return [size_case(256, 255, THR[:1], S["size0"]), size_case(257, 256, THR, S["size1"]), size_case(512, 257, THR, S["size2"]),
            size_case(512, 1000, THR16, S["size3"], tmax=0.95), ties_case(S["ties"]), invalid_case(S["invalid"]), counts_case(S["counts"])]


@functools.lru_cache(maxsize=None)
def all_cases():
    return [match_cases() + (THR, "cases"), tiny_case() + (THR, "tiny")] + edge_cases()


@functools.lru_cache(maxsize=None)
def all_band():
    """`band` over the committed cases, old and new -> (band, fp64 pair list per case of all_cases())"""
    return band(all_cases())


def same_rows(gl_b, gb_b, g, h):
    """two ground-truth rows bit-identical (class and box): the one condition under which two candidates may tie"""
    return gl_b[g] == gl_b[h] and gb_b[g].tobytes() == gb_b[h].tobytes()


def edge_claims(case, tp, bi, bg):
    """what an edge case is there to show, asserted on a result (the reference's on the CPU, the device's on the GPU)"""
    det, count, gl, gb, mk, nc, thr, name = case
    full = (1 << len(thr)) - 1
    if name.startswith("size"):
        n_cap, max_det = gl.shape[1], det.shape[1]
        assert mk[0].all() and count[0] == max_det and (bg[0] >= 0).all() and bg[0, max_det - 1] == n_cap - 1 and (tp[0] == full).any()
        assert (bg[1, count[1]:] == -1).all() and not tp[1, count[1]:].any() and not bi[1, count[1]:].any() and tp.max() <= full
    elif name == "ties":
        assert same_rows(gl[0], gb[0], *TIE_GT) and all(bg[0, d] == TIE_GT[0] for d in TIE_DETS) and (bg[0] != TIE_GT[1]).all()
        for d, e, g in ((TIE_NEXT[0], TIE_NEXT[0] + 1, TIE_NEXT[1]), TIE_LANE):
            assert det[0, d, [0, 1, 2, 3, 5, 6]].tobytes() == det[0, e, [0, 1, 2, 3, 5, 6]].tobytes()
            assert bg[0, d] == bg[0, e] == g and bi[0, d] == bi[0, e] > 0.5 and tp[0, d] & 1 and tp[0, e] == 0
        assert TIE_LANE[0] % 256 == TIE_LANE[1] % 256
    elif name == "invalid-rows":
        for d in BAD_DET:
            assert d < count[0] and (bg[0, d], bi[0, d], tp[0, d]) == (-1, 0, 0), BAD_DET[d]
        assert mk[0, list(BAD_GT)].all() and not np.isin(bg[0], list(BAD_GT)).any()
        live = [d for d in range(count[0]) if d not in BAD_DET]
        assert (bg[0, live] >= 0).all() and tp[0, live].any()
    elif name == "counts":
        assert count.tolist() == [det.shape[1] + 7, -4] and (bg[0] >= 0).all() and tp[0].any()
        assert (bg[1] == -1).all() and not tp[1].any() and not bi[1].any()
