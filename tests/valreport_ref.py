"""CPU side of the validation-report tests (ops.val_confusion, metrics.pr_curves, train.Validator(report=True)) -- not the product, nothing here
touches the GPU.  Written from the rules (Ultralytics 8.3.x `ConfusionMatrix.process_batch` for OBB and the curve half of `ap_per_class`, restated
from recall: UNPINNED), in fp64 and plain loops, with no helper of the product or of the other reference modules:

  probiou_row(g, d)               batch_probiou's covariance form (eps 1e-7) of one detection against a list of ground truths, fp64
  confusion(...)                  the confusion rule -> int64 [nc+1, nc+1]
  margins(...)                    how far a case's decisions are from flipping: the least |IoU - iou_thr| of a candidate pair and the least gap between
                                  the IoUs competing for one detection or one ground truth (exact ties -- duplicated boxes -- excepted and counted)
  pr_curves(...)                  the P / R / F1 curves and the operating point, loops over a 1000-point grid
  confusion_cases()               the data of the confusion tests (generated, plus the hand-built named ones), shared by the CPU margin test and
                                  the GPU test: {id: (det, count, gt_labels, gt_bboxes, mask_gt, nc)}"""
import functools
import itertools
import math

import numpy as np

CM_CONF, CM_IOU = 0.25, 0.45
GAP = 2.5e-3  # the generator keeps competing IoUs this far apart; the tests ask for 1e-3
SEED = 1  # chosen so that test_valreport_cpu's margin assertions hold for EVERY generated case (they are asserted, not assumed)


# ---------------------------------------------------------------------------------------------------------------- the confusion rule
def probiou_row(g, d):
    """g [n,5] ground truths, d [5] one detection, (x, y, w, h, theta), fp64 -> [n]"""
    g, d = np.asarray(g, np.float64).reshape(-1, 5), np.asarray(d, np.float64)
    eps = 1e-7

    def cov(w, h, t):
        a, b = w * w / 12.0, h * h / 12.0
        c, s = np.cos(t), np.sin(t)
        return a * c * c + b * s * s, a * s * s + b * c * c, (a - b) * c * s

    a1, b1, c1 = cov(g[:, 2], g[:, 3], g[:, 4])
    a2, b2, c2 = cov(d[2], d[3], d[4])
    A, B, C = a1 + a2, b1 + b2, c1 + c2
    dx, dy = g[:, 0] - d[0], g[:, 1] - d[1]
    with np.errstate(all="ignore"):
        den = A * B - C * C + eps
        t1 = (A * dy * dy + B * dx * dx) / den * 0.25
        t2 = (C * (-dx) * dy) / den * 0.5
        det1, det2 = np.maximum(a1 * b1 - c1 * c1, 0.0), max(a2 * b2 - c2 * c2, 0.0)
        t3 = np.log((A * B - C * C) / (4.0 * np.sqrt(det1 * det2) + eps) + eps) * 0.5
        bd = np.clip(t1 + t2 + t3, eps, 100.0)
        return 1.0 - np.sqrt(1.0 - np.exp(-bd) + eps)


def _valid_gts(gl_b, gb_b, mk_b, nc):
    return [g for g in range(len(gl_b)) if mk_b[g] and 0 <= int(gl_b[g]) < nc and bool(np.isfinite(np.asarray(gb_b[g], np.float64)).all())]


def _candidates(det_b, count_b, nc, conf_thr):
    out = []
    for d in range(min(max(int(count_b), 0), len(det_b))):
        row = np.asarray(det_b[d], np.float64)
        if row[4] > conf_thr and 0 <= row[5] < nc and bool(np.isfinite(row[[0, 1, 2, 3, 6]]).all()):  # (NaN fails every comparison)
            out.append(d)
    return out


def _image(det_b, count_b, gl_b, gb_b, mk_b, nc, conf_thr, iou_thr):
    """-> (candidates [d], valid ground truths [g], {d: (picked g or -1, its IoU)}, {d: IoUs against the valid ground truths})"""
    gs = _valid_gts(gl_b, gb_b, mk_b, nc)
    cands = _candidates(det_b, count_b, nc, conf_thr)
    pick, ious = {}, {}
    for d in cands:
        v = probiou_row(np.asarray(gb_b, np.float64)[gs], np.asarray(det_b[d], np.float64)[[0, 1, 2, 3, 6]]) if gs else np.zeros(0)
        ious[d] = v
        best, bg = iou_thr, -1
        for g, iou in zip(gs, v):
            if iou > best:  # strict: above the threshold; a tie keeps the lower index
                best, bg = iou, g
        pick[d] = (bg, best)
    return cands, gs, pick, ious


def confusion(det, count, gl, gb, mk, nc, conf_thr=CM_CONF, iou_thr=CM_IOU):
    """-> int64 [nc+1, nc+1]: [pred, gt] per kept pair, [pred, nc] per candidate without a ground truth, [nc, gt] per ground truth without a detection"""
    m = np.zeros((nc + 1, nc + 1), np.int64)
    for b in range(det.shape[0]):
        cands, gs, pick, _ = _image(det[b], count[b], gl[b], gb[b], mk[b], nc, conf_thr, iou_thr)
        keeper = {}
        for d in cands:  # ascending index: a later detection takes a ground truth only with a strictly larger IoU
            g, iou = pick[d]
            if g >= 0 and (g not in keeper or iou > keeper[g][1]):
                keeper[g] = (d, iou)
        for d in cands:
            g = pick[d][0]
            pc = int(det[b, d, 5])
            if g >= 0 and keeper[g][0] == d:
                m[pc, int(gl[b, g])] += 1
            else:
                m[pc, nc] += 1
        for g in gs:
            if g not in keeper:
                m[nc, int(gl[b, g])] += 1
    return m


def margins(det, count, gl, gb, mk, nc, conf_thr=CM_CONF, iou_thr=CM_IOU):
    """-> (least |IoU - iou_thr| over the candidate pairs, least gap between two IoUs above iou_thr competing for one detection or for one ground
    truth, number of exact ties among those, least |conf - conf_thr| over the live, otherwise valid detections)"""
    thr_m, gap_m, ties, conf_m = math.inf, math.inf, 0, math.inf
    for b in range(det.shape[0]):
        for d in range(min(max(int(count[b]), 0), det.shape[1])):
            c = float(det[b, d, 4])
            if math.isfinite(c):
                conf_m = min(conf_m, abs(c - conf_thr))
        cands, gs, pick, ious = _image(det[b], count[b], gl[b], gb[b], mk[b], nc, conf_thr, iou_thr)
        claims = {}
        for d in cands:
            v = ious[d]
            if len(v):
                thr_m = min(thr_m, float(np.abs(v - iou_thr).min()))
            above = np.sort(v[v > iou_thr])[::-1]
            if len(above) >= 2:
                if above[0] == above[1]:
                    ties += 1
                else:
                    gap_m = min(gap_m, float(above[0] - above[1]))
            if pick[d][0] >= 0:
                claims.setdefault(pick[d][0], []).append(pick[d][1])
        for v in claims.values():
            v = sorted(v, reverse=True)
            if len(v) >= 2:
                if v[0] == v[1]:
                    ties += 1
                else:
                    gap_m = min(gap_m, v[0] - v[1])
    return thr_m, gap_m, ties, conf_m


# ---------------------------------------------------------------------------------------------------------------- the curves
def _interp_desc(x, conf, val, left):
    """numpy's interp(-x, -conf, val, left=left) for conf in non-increasing order, by a scan: above the largest confidence `left`, at or below the
    least the last value, otherwise linear between the LAST detection with conf >= x and the one after it"""
    n = len(conf)
    if x > conf[0]:
        return left
    j = 0
    while j + 1 < n and conf[j + 1] >= x:
        j += 1
    if j == n - 1 or conf[j] == x:
        return val[j]
    return val[j] + (val[j + 1] - val[j]) * (conf[j] - x) / (conf[j] - conf[j + 1])


def pr_curves(tp, conf, pred_cls, target_cls, nc):
    tp, conf, pred_cls, target_cls = np.asarray(tp, bool), np.asarray(conf, np.float64), np.asarray(pred_cls), np.asarray(target_cls)
    order = sorted(range(len(conf)), key=lambda i: -conf[i])  # Python's sort is stable
    classes = sorted({int(c) for c in target_cls})
    N = 1000
    xs = [i / (N - 1) for i in range(N)]
    P, R, F = np.zeros((len(classes), N)), np.zeros((len(classes), N)), np.zeros((len(classes), N))
    for ci, c in enumerate(classes):
        n_gt = int((target_cls == c).sum())
        idx = [i for i in order if int(pred_cls[i]) == c]
        if not idx:
            continue
        t = f = 0
        rec, pre, cf = [], [], []
        for i in idx:
            t, f = t + int(tp[i, 0]), f + int(not tp[i, 0])
            rec.append(t / (n_gt + 1e-16)); pre.append(t / (t + f)); cf.append(float(conf[i]))
        for k, x in enumerate(xs):
            R[ci, k], P[ci, k] = _interp_desc(x, cf, rec, 0.0), _interp_desc(x, cf, pre, 1.0)
            F[ci, k] = 2 * P[ci, k] * R[ci, k] / (P[ci, k] + R[ci, k] + 1e-16)
    if not classes:
        z = np.zeros(0)
        return {"x": np.asarray(xs), "p_curve": P, "r_curve": R, "f1_curve": F, "classes": np.zeros(0, np.int64), "conf_best": 0.0, "p": z, "r": z, "f1": z,
                "mp": 0.0, "mr": 0.0, "smoothed": np.zeros(N)}
    mean = [sum(F[ci, k] for ci in range(len(classes))) / len(classes) for k in range(N)]
    half = 50  # 101 taps over edge-padded values
    sm = [sum(mean[min(max(k + o, 0), N - 1)] for o in range(-half, half + 1)) / (2 * half + 1) for k in range(N)]
    i = max(range(N), key=lambda k: (sm[k], -k))  # the first maximum
    return {"x": np.asarray(xs), "p_curve": P, "r_curve": R, "f1_curve": F, "classes": np.asarray(classes, np.int64), "conf_best": xs[i], "p": P[:, i],
            "r": R[:, i], "f1": F[:, i], "mp": float(P[:, i].mean()), "mr": float(R[:, i].mean()), "smoothed": np.asarray(sm)}


def pr_case(kind, seed=0):
    """-> (tp bool [n,10], conf, pred_cls, target_cls, nc) for the kinds of test_valreport_cpu"""
    rng = np.random.RandomState(100 + seed)
    nc = 1 if kind == "one_class" else 5
    n = 0 if kind == "no_detections" else 60
    m = 0 if kind == "no_targets" else 25
    target = rng.randint(0, nc, m)
    if kind == "class_without_detections" and m:
        target[:3] = 4
    pred = rng.randint(0, nc - 1 if kind == "class_without_detections" else nc, n).astype(np.float32)
    conf = rng.uniform(0.02, 0.98, n)
    if kind == "ties":
        conf = np.round(conf * 8) / 8  # nine distinct values, some of them grid points of x
    tp = rng.uniform(size=(n, 10)) < np.linspace(0.7, 0.1, 10)[None, :]
    return tp, conf.astype(np.float32), pred, target.astype(np.int32), nc


PR_KINDS = ["random", "ties", "one_class", "class_without_detections", "no_detections", "no_targets"]


# ---------------------------------------------------------------------------------------------------------------- confusion cases
def _jitter(rng, g, t):
    """a copy of box g moved by t x its extent in a random direction, sides within 5 %, angle within 0.05 rad: IoU ~ 1 - sqrt(1 - exp(-1.5 t^2))"""
    a = rng.uniform(0, 2 * np.pi)
    c, s = np.cos(g[4]), np.sin(g[4])
    du, dv = t * g[2] * np.cos(a), t * g[3] * np.sin(a)
    return [g[0] + du * c - dv * s, g[1] + du * s + dv * c, g[2] * rng.uniform(0.95, 1.05), g[3] * rng.uniform(0.95, 1.05), g[4] + rng.uniform(-0.05, 0.05)]


def _empty(B, max_det, n_cap):
    """every row garbage until written: NaN boxes, classes far outside [0, nc), masks off"""
    det = np.full((B, max_det, 7), np.nan, np.float32)
    det[..., 5] = 1e6
    gl = np.full((B, n_cap), 10 ** 6, np.int32)
    gb = np.full((B, n_cap, 5), np.nan, np.float32)
    return det, np.zeros(B, np.int32), gl, gb, np.zeros((B, n_cap), bool)


def _fill_image(rng, det_b, gl_b, gb_b, mk_b, nc, kind):
    """one image.  kind 0: general; 1: count 0; 2: count past max_det (every row live); 3: every detection under the confidence threshold;
    4: no valid ground truth.  -> count"""
    max_det, n_cap = det_b.shape[0], gl_b.shape[0]
    side = int(math.ceil(math.sqrt(n_cap)))
    n_gt = 0 if kind == 4 else int(rng.randint(max(1, n_cap // 2), n_cap + 1))
    rows = np.sort(rng.permutation(n_cap)[:n_gt])  # the unmasked rows, masked garbage between them
    cells = rng.permutation(side * side)[:n_gt]
    for g, cell in zip(rows, cells):
        gb_b[g] = [100.0 * (cell % side) + 50, 100.0 * (cell // side) + 50, rng.uniform(20, 40), rng.uniform(20, 40), rng.uniform(-0.7, 2.3)]
        gl_b[g] = rng.randint(0, nc)
        mk_b[g] = True
    good = list(rows)
    if n_gt >= 6:  # an unmasked row of a class outside [0, nc), one with a NaN side (both count nowhere), and an exact copy of a box (the tie)
        gl_b[good.pop(1)] = nc
        gb_b[good.pop(2), 2] = np.nan
        gb_b[good[3]] = gb_b[good[0]]
        if nc > 1:
            gl_b[good[3]] = (gl_b[good[0]] + 1) % nc
    if kind == 1:
        return 0
    n_live = max_det if kind == 2 else int(rng.randint(max(1, max_det // 2), max_det + 1))
    dets, taken = [], {}
    for _ in range(n_live):
        lo = kind == 3 or rng.uniform() < 0.15
        conf = rng.uniform(0.01, 0.2) if lo else rng.uniform(0.3, 0.99)
        u = rng.uniform()
        if good and u < 0.85:
            g = good[rng.randint(len(good))]
            cls = int(gl_b[g]) if rng.uniform() < 0.7 else int(rng.randint(0, nc))
            for _ in range(40):  # keep the IoUs that compete for one ground truth GAP apart (the guarantee test_valreport_cpu asserts from outside)
                t = rng.uniform(0.05, 0.33) if rng.uniform() < 0.7 else rng.uniform(0.75, 1.3)
                box = np.asarray(_jitter(rng, gb_b[g].astype(np.float64), t), np.float32)
                iou = float(probiou_row(gb_b[g], box)[0])
                if abs(iou - CM_IOU) >= 0.05 and all(abs(iou - v) >= GAP for v in taken.setdefault(int(g), [])):
                    taken[int(g)].append(iou)
                    dets.append([float(v) for v in box] + [conf, cls])
                    break
            else:
                u = 1.0
        if not (good and u < 0.85):  # off the grid: background
            dets.append([-500.0 - 100 * rng.randint(0, 50), -500.0 - 100 * rng.randint(0, 50), rng.uniform(20, 40), rng.uniform(20, 40), rng.uniform(-0.7, 2.3),
                         conf, int(rng.randint(0, nc))])
    if n_live >= 8 and kind != 3:
        dets[1][:5] = dets[0][:5]          # an exact copy of a detection's box: the lower index keeps the ground truth
        dets[1][5] = dets[0][5] = 0.9
        dets[3][6] = nc                    # live rows that count nowhere: a class outside [0, nc), a NaN side, a NaN confidence
        dets[4][2] = np.nan
        dets[5][5] = np.nan
    dets.sort(key=lambda r: -r[5] if r[5] == r[5] else 1.0)  # score order, as decode_nms leaves them (Python's sort is stable)
    for d, r in enumerate(dets):
        det_b[d] = [r[0], r[1], r[2], r[3], r[5], r[6], r[4]]
    return max_det + 7 if kind == 2 else n_live


def generated_case(B, max_det, n_cap, nc, seed=SEED):
    rng = np.random.RandomState(seed * 1000003 + B * 7919 + max_det * 31 + n_cap * 3 + nc)
    det, count, gl, gb, mk = _empty(B, max_det, n_cap)
    for b in range(B):
        count[b] = _fill_image(rng, det[b], gl[b], gb[b], mk[b], nc, b % 5)
    return det, count, gl, gb, mk, nc


def _hand(nc, dets, gts, max_det=4, n_cap=4):
    """dets: [(x, y, w, h, theta, conf, cls)], gts: [(x, y, w, h, theta, cls)] -> a one-image case"""
    det, count, gl, gb, mk = _empty(1, max_det, n_cap)
    for d, r in enumerate(dets):
        det[0, d] = [r[0], r[1], r[2], r[3], r[5], r[6], r[4]]
    for g, r in enumerate(gts):
        gb[0, g], gl[0, g], mk[0, g] = r[:5], r[5], True
    count[0] = len(dets)
    return det, count, gl, gb, mk, nc


def named_cases():
    """hand-built, each with the matrix it must give ([pred, gt], nc = 3: index 3 = background)"""
    G0, G1 = (50, 50, 30, 20, 0.3, 1), (250, 50, 30, 20, 0.3, 2)
    on = lambda g, dx, conf, cls: (g[0] + dx, g[1], g[2], g[3], g[4], conf, cls)

    def z(cells):
        m = np.zeros((4, 4), np.int64)
        for k, v in cells.items():
            m[k] = v
        return m

    return {
        "two_on_one": (_hand(3, [on(G0, 3.0, 0.9, 1), on(G0, 1.0, 0.8, 1)], [G0, G1]), z({(1, 1): 1, (1, 3): 1, (3, 2): 1})),   # the closer one keeps it
        "off_diagonal": (_hand(3, [on(G0, 1.0, 0.9, 0)], [G0]), z({(0, 1): 1})),
        "duplicate_dets": (_hand(3, [on(G0, 2.0, 0.9, 1), on(G0, 2.0, 0.9, 2)], [G0]), z({(1, 1): 1, (2, 3): 1})),              # the lower index keeps it
        "duplicate_gts": (_hand(3, [on(G0, 2.0, 0.9, 1)], [G0, G0[:5] + (2,)]), z({(1, 1): 1, (3, 2): 1})),                      # the lower index is picked
        "under_conf": (_hand(3, [on(G0, 1.0, 0.2, 1), on(G1, 1.0, 0.25, 2)], [G0, G1]), z({(3, 1): 1, (3, 2): 1})),              # conf > 0.25 is strict
        "count_zero": (_hand(3, [], [G0]), z({(3, 1): 1})),
        "garbage_rows": (_hand(3, [on(G0, 1.0, 0.9, 1)], [G0]), z({(1, 1): 1})),                                                  # NaN / class 1e6 past the counts
    }


GEN_PARAMS = list(itertools.product((1, 5), (1, 40, 300), (1, 64, 512), (1, 12)))  # (B, max_det, n_cap, nc)
gen_id = lambda p: "B%d-det%d-cap%d-nc%d" % p


@functools.lru_cache(maxsize=None)
def confusion_cases():
    """{id: case} of every generated and named case; computed once and shared"""
    out = {gen_id(p): generated_case(*p) for p in GEN_PARAMS}
    out.update({k: v[0] for k, v in named_cases().items()})
    return out


@functools.lru_cache(maxsize=None)
def confusion_refs():
    """{id: the restatement's matrix}: computed once, shared by the tests, never written to"""
    out = {k: confusion(*c) for k, c in confusion_cases().items()}
    for m in out.values():
        m.setflags(write=False)
    return out
