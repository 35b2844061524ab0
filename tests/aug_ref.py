"""numpy / fp64 restatement of the training-batch augmentation (include/obbhip.h, "f1 (training batches)"), by an independent route: the mosaic canvas
is MATERIALISED here and then warped as a whole image, where the device gathers every tap through the quadrant arithmetic; the HSV tables are built
in float64 with np.rint as cv2 builds them, where the device uses closed-form integer quotients; the labels are walked one by one in Python floats.
Ultralytics 8.3.x and cv2 restated from recall (neither is installed): UNPINNED.  The record layout is read from the product's own `augment.REC`.

`label_ref(..., bug=...)` plants one of six mistakes (BUGS) for the tests that show the sanity checks catch them; `margins=` collects, per discrete
decision, (kind, relative margin) so that the CPU suite can assert no committed GPU case sits within rounding of a decision.

`label_cases()` and `label_edge_cases()` are the label cases of the GPU suite (the second: the label kernel's launch and domain edges); the builders
beside them (`centre_table`, `offcanvas_table`, `colour_pool` / `colour_table`) are the pixel cases of tests/test_gpu_batch_edges.py."""
import functools
import math

import numpy as np

BORDER = 114
TIE = 1e-7  # a later edge replaces the running minimum-area rectangle only when it is smaller by more than this (relative)
BUGS = ("no_pad", "no_canvas_clip", "flip_before_M", "swap_wh", "area_inverted", "M_for_inverse")


# ---------------------------------------------------------------- pixels
def canvas_of(pool, rec):
    """The canvas the device never builds: [S, S, C] uint8"""
    s = pool.shape[1]
    if not rec["flags"] & 1:
        return pool[rec["src"][0]].copy()
    S, xc, yc = 2 * s, int(rec["xc"]), int(rec["yc"])
    cv = np.full((S, S, pool.shape[3]), BORDER, np.uint8)
    # _mosaic4 for equal-sized images: quadrant q shows its tile placed with one corner at the centre, cut at the canvas
    for q, (x1, y1, x2, y2) in enumerate([(max(xc - s, 0), max(yc - s, 0), xc, yc), (xc, max(yc - s, 0), min(xc + s, S), yc),
                                          (max(xc - s, 0), yc, xc, min(S, yc + s)), (xc, yc, min(xc + s, S), min(S, yc + s))]):
        padw, padh = (xc if q & 1 else xc - s), (yc if q & 2 else yc - s)
        cv[y1:y2, x1:x2] = pool[rec["src"][q]][y1 - padh:y2 - padh, x1 - padw:x2 - padw]
    return cv


def _fix(v):
    return np.rint(np.clip(v, -536870912.0, 536870912.0)).astype(np.int64)


def warp(canvas, inv, s):
    """cv2.warpAffine(canvas, M, (s, s), INTER_LINEAR, borderValue=114) in its fixed point, given the inverse map [6]"""
    S = canvas.shape[0]
    x = np.arange(s, dtype=np.float64)
    m = [np.float64(v) for v in inv]
    X = (_fix(m[0] * x * 1024.0)[None, :] + _fix((m[1] * x + m[2]) * 1024.0)[:, None] + 16) >> 5
    Y = (_fix(m[3] * x * 1024.0)[None, :] + _fix((m[4] * x + m[5]) * 1024.0)[:, None] + 16) >> 5
    ix, iy, fx, fy = np.clip(X >> 5, -2, S), np.clip(Y >> 5, -2, S), (X & 31)[..., None], (Y & 31)[..., None]
    pad = np.full((S + 4, S + 4, canvas.shape[2]), BORDER, np.int64)
    pad[2:S + 2, 2:S + 2] = canvas
    t00, t01, t10, t11 = pad[iy + 2, ix + 2], pad[iy + 2, ix + 3], pad[iy + 3, ix + 2], pad[iy + 3, ix + 3]
    acc = 32 * (32 - fx) * (32 - fy) * t00 + 32 * fx * (32 - fy) * t01 + 32 * (32 - fx) * fy * t10 + 32 * fx * fy * t11
    return ((acc + 16384) >> 15).astype(np.uint8)


_I = np.arange(256, dtype=np.float64)
with np.errstate(divide="ignore"):
    SDIV = np.where(_I > 0, np.rint((255 << 12) / np.where(_I > 0, _I, 1)), 0).astype(np.int64)
    HDIV = np.where(_I > 0, np.rint((180 << 12) / (6.0 * np.where(_I > 0, _I, 1))), 0).astype(np.int64)


def bgr2hsv(b, g, r):
    b, g, r = (a.astype(np.int64) for a in (b, g, r))
    v = np.maximum(b, np.maximum(g, r))
    diff = v - np.minimum(b, np.minimum(g, r))
    sat = (diff * SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + 2048) >> 12
    return np.where(h < 0, h + 180, h), sat, v


def hsv2bgr(h, sat, v):
    f32 = np.float32
    hf = h.astype(f32) * (f32(6) / f32(180))
    sf, vf = sat.astype(f32) * (f32(1) / f32(255)), v.astype(f32) * (f32(1) / f32(255))
    sec = np.floor(hf).astype(np.int64)
    f = hf - sec.astype(f32)
    bad = (sec < 0) | (sec >= 6)
    sec, f = np.where(bad, 0, sec), np.where(bad, f32(0), f)
    one = f32(1)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))])
    assert tab.dtype == np.float32
    sector = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    out = []
    for k in range(3):
        val = np.take_along_axis(tab, sector[sec, k][None], 0)[0]
        out.append(np.clip(np.rint(val * f32(255)), 0, 255).astype(np.uint8))
    return out


def hsv_apply(img, lut, bgr=True):
    """the HSV gains on [..., C >= 3] uint8 in place: integer BGR -> HSV, the three tables, fp32 HSV -> BGR; a fourth channel stays"""
    cb, cr = (0, 2) if bgr else (2, 0)
    h, sa, v = bgr2hsv(img[..., cb], img[..., 1], img[..., cr])
    nb, ng, nr = hsv2bgr(lut[h], lut[256 + sa], lut[512 + v])
    img[..., cb], img[..., 1], img[..., cr] = nb, ng, nr
    return img


def tiles_ref(pool, table, bgr=True, swap_rb=False):
    """-> uint8 [B, s, s, C]: what obb_aug_tiles must give, bit for bit"""
    s = pool.shape[1]
    out = np.empty((len(table), s, s, pool.shape[3]), np.uint8)
    for b, rec in enumerate(table):
        img = warp(canvas_of(pool, rec), rec["inv"], s)
        if rec["flags"] & 2:
            img = img[:, ::-1]
        if rec["flags"] & 4:
            img = img[::-1]
        img = img.copy()
        if rec["flags"] & 8:
            hsv_apply(img, rec["lut"], bgr)
        if swap_rb:
            img[..., [0, 2]] = img[..., [2, 0]]
        out[b] = img
    return out


# ---------------------------------------------------------------- labels
def xywhr_corners(box):
    """(x, y, w, h, theta) -> [4, 2] corners, w along (cos, sin)"""
    x, y, w, h, t = (float(v) for v in box)
    c, s_ = math.cos(t), math.sin(t)
    u, n = np.array([c, s_]) * w / 2, np.array([-s_, c]) * h / 2
    ctr = np.array([x, y])
    return np.array([ctr + u + n, ctr - u + n, ctr - u - n, ctr + u - n])


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(pts):
    """monotone chain, counter-clockwise in (x, y), collinear points dropped, starting at the lexicographic minimum"""
    p = sorted((float(x), float(y)) for x, y in pts)
    h = []
    for q in p:
        while len(h) >= 2 and _cross(h[-2], h[-1], q) <= 0:
            h.pop()
        h.append(q)
    t = len(h) + 1
    for q in reversed(p[:-1]):
        while len(h) >= t and _cross(h[-2], h[-1], q) <= 0:
            h.pop()
        h.append(q)
    return h[:-1]


def clip_square(poly, s):
    """Sutherland-Hodgman against [0, s]^2; a crossing point gets the bound itself as its clipped coordinate"""
    for axis, bound, lower in ((0, 0.0, True), (0, float(s), False), (1, 0.0, True), (1, float(s), False)):
        out = []
        for i, a in enumerate(poly):
            b = poly[(i + 1) % len(poly)]
            ia = a[axis] >= bound if lower else a[axis] <= bound
            ib = b[axis] >= bound if lower else b[axis] <= bound
            if ia:
                out.append(a)
            if ia != ib:
                t = (bound - a[axis]) / (b[axis] - a[axis])
                o = 1 - axis
                v = a[o] + t * (b[o] - a[o])
                out.append((bound, v) if axis == 0 else (v, bound))
        poly = out
        if not poly:
            break
    return poly


def min_area_rect(poly, margins=None, bug=None):
    """-> (x, y, w, h, theta), theta in [0, pi/2), w along (cos theta, sin theta); the first edge in order wins a tie
    (areas within TIE of each other: every edge of a triangle gives the same area, so ties are the rule, not the exception).  None without a usable edge."""
    P = np.asarray(poly, np.float64)
    best = None
    for i in range(len(P)):
        d = P[(i + 1) % len(P)] - P[i]
        l2 = float(d[0] * d[0] + d[1] * d[1])
        if margins is not None and l2 != 0.0:
            margins.append(("edge", _rel(l2, 1e-12)))
        if l2 < 1e-12:
            continue
        ux, uy = d / math.sqrt(l2)
        pu, pn = P[:, 0] * ux + P[:, 1] * uy, P[:, 1] * ux - P[:, 0] * uy
        area = (pu.max() - pu.min()) * (pn.max() - pn.min())
        if best is not None and margins is not None:
            margins.append(("tie", _rel(area, best[0] * (1.0 - TIE))))
        if best is None or area < best[0] * (1.0 - TIE):
            best = (area, ux, uy, pu.min(), pu.max(), pn.min(), pn.max())
    if best is None:
        return None
    area, ux, uy, u0, u1, n0, n1 = best
    if margins is not None:
        for v in (ux, uy):
            if v != 0.0:
                margins.append(("quadrant", abs(v)))
    cu, cn = 0.5 * (u0 + u1), 0.5 * (n0 + n1)
    cx, cy = cu * ux - cn * uy, cu * uy + cn * ux
    w, h = u1 - u0, n1 - n0
    if ux > 0 and uy >= 0:
        c, sn, odd = ux, uy, False
    elif ux <= 0 and uy > 0:
        c, sn, odd = uy, -ux, True
    elif ux < 0 and uy <= 0:
        c, sn, odd = -ux, -uy, False
    else:
        c, sn, odd = -uy, ux, True
    if odd:
        w, h = h, w
    if bug == "swap_wh":
        w, h = h, w
    return cx, cy, w, h, math.atan2(sn, c)


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def _separation(H, s):
    """the widest gap between the convex hull H (counter-clockwise) and [0, s]^2 along the tile's axes and the hull's edge normals: positive exactly
    when the two are disjoint (separating axes of two convex polygons).  The hull's box alone says nothing about a turned label beside a tile corner."""
    gap = max(0.0 - H[:, 0].max(), H[:, 0].min() - s, 0.0 - H[:, 1].max(), H[:, 1].min() - s)
    corners = np.array([(0.0, 0.0), (s, 0.0), (s, s), (0.0, s)])
    for i in range(len(H)):
        d = H[(i + 1) % len(H)] - H[i]
        gap = max(gap, float(((corners - H[i]) @ (np.array([d[1], -d[0]]) / math.hypot(d[0], d[1]))).min()))  # (dy, -dx): the outward normal
    return gap


def candidate_ref(rec, q, row, s, wh_thr=2.0, ar_thr=100.0, area_thr=0.01, margins=None, bug=None):
    """one (quadrant, label row) -> (class, (x, y, w, h, theta)) or None"""
    mosaic = bool(rec["flags"] & 1)
    S = 2.0 * s if mosaic else float(s)
    padx = pady = 0.0
    if mosaic and bug != "no_pad":
        padx = float(rec["xc"] if q & 1 else rec["xc"] - s)
        pady = float(rec["yc"] if q & 2 else rec["yc"] - s)
    M = [float(v) for v in (rec["inv"] if bug == "M_for_inverse" else rec["fwd"])]
    lr, ud = bool(rec["flags"] & 2), bool(rec["flags"] & 4)
    before, after = [], []
    for k in range(4):
        x, y = float(row[1 + 2 * k]) * s + padx, float(row[2 + 2 * k]) * s + pady
        if bug != "no_canvas_clip":
            x, y = min(max(x, 0.0), S), min(max(y, 0.0), S)
        before.append((x, y))
        if bug == "flip_before_M":
            x, y = (s - x if lr else x), (s - y if ud else y)
        tx, ty = (M[0] * x + M[1] * y) + M[2], (M[3] * x + M[4] * y) + M[5]
        if bug != "flip_before_M":
            tx, ty = (s - tx if lr else tx), (s - ty if ud else ty)
        after.append((tx, ty))
    B, A = np.array(before), np.array(after)
    w1, h1 = (B[:, 0].max() - B[:, 0].min()) * float(rec["scale"]), (B[:, 1].max() - B[:, 1].min()) * float(rec["scale"])
    Ac = np.clip(A, 0.0, float(s))
    w2, h2 = Ac[:, 0].max() - Ac[:, 0].min(), Ac[:, 1].max() - Ac[:, 1].min()
    ar = max(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
    ratio = w2 * h2 / (w1 * h1 + 1e-16)
    if bug == "area_inverted":
        ratio = w1 * h1 / (w2 * h2 + 1e-16)
    if margins is not None:
        margins += [("wh", _rel(w2, wh_thr)), ("wh", _rel(h2, wh_thr)), ("aspect", _rel(ar, ar_thr))]
        if w2 > 0 and h2 > 0:
            margins.append(("area", _rel(ratio, area_thr)))
    if not (w2 > wh_thr and h2 > wh_thr and ratio > area_thr and ar < ar_thr):
        return None
    hl = hull(after)
    if len(hl) < 3:
        return None
    poly = clip_square(hl, s)
    if margins is not None:  # an empty clip: the gap between the hull and the tile, or the area that is left, over the tile's
        H = np.array(hl)
        if len(poly) < 3:
            margins.append(("clip", max(_separation(H, s), 0.0) / s))
        else:
            Q = np.array(poly)
            margins.append(("clip", 0.5 * abs(np.dot(Q[:, 0], np.roll(Q[:, 1], -1)) - np.dot(Q[:, 1], np.roll(Q[:, 0], -1))) / (s * s)))
    if len(poly) < 3:
        return None
    r = min_area_rect(poly, margins, bug)
    if r is None:
        return None
    if margins is not None:
        margins += [("2px", _rel(r[2], 2.0)), ("2px", _rel(r[3], 2.0))]
    if r[2] < 2.0 or r[3] < 2.0:
        return None
    return int(row[0]), r


def labels_ref(pool_labels, pool_counts, table, s, n_cap, wh_thr=2.0, ar_thr=100.0, area_thr=0.01, margins=None, bug=None):
    """-> (gt_labels int32 [B,n_cap], gt_bboxes float64 [B,n_cap,5], mask bool [B,n_cap], count int32 [B], rows): what obb_aug_labels must give (the
    boxes here in fp64); rows = every survivor as (b, class, x, y, w, h, theta), also those past n_cap"""
    B, Lmax = len(table), pool_labels.shape[1]
    gl, gb = np.zeros((B, n_cap), np.int32), np.zeros((B, n_cap, 5))
    mk, cnt, rows = np.zeros((B, n_cap), bool), np.zeros(B, np.int32), []
    for b, rec in enumerate(table):
        k = 0
        for q in range(4 if rec["flags"] & 1 else 1):
            t = int(rec["src"][q])
            for l in range(min(max(int(pool_counts[t]), 0), Lmax)):
                r = candidate_ref(rec, q, pool_labels[t, l], s, wh_thr, ar_thr, area_thr, margins, bug)
                if r is None:
                    continue
                rows.append((b, r[0]) + tuple(r[1]))
                if k < n_cap:
                    gl[b, k], gb[b, k], mk[b, k] = r[0], r[1], True
                k += 1
        cnt[b] = k
    return gl, gb, mk, cnt, rows


# ---------------------------------------------------------------- the committed GPU cases (shared by the GPU tests and the CPU margin check)
def _aug():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import augment
    return augment


def random_pool(N, s, C, seed):
    """tiles with every hard colour in them: pure greys, saturated primaries, 0 and 255, and noise"""
    rng = np.random.RandomState(seed)
    pool = rng.randint(0, 256, (N, s, s, C)).astype(np.uint8)
    k = s // 4
    pool[0, :k, :k] = np.linspace(0, 255, k).astype(np.uint8)[None, :, None]  # greys
    for i, col in enumerate([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]):
        pool[1, :k, i * (s // 6):(i + 1) * (s // 6), :3] = col
    pool[2, :k] = 0
    pool[2, k:2 * k] = 255
    return pool


def pixel_tables(N, s, B, mosaic, seed):
    """B records that together walk the corners of the domain: centres at the ends of their range, scale 0.5 / 1.5, translation at both extremes, a
    17-degree rotation, each flip, HSV off and at both gain extremes"""
    A = _aug()
    rng = np.random.RandomState(seed)
    S = 2 * s if mosaic else s
    centres = [(s // 2, s // 2), (3 * s // 2 - 1, 3 * s // 2 - 1), (s // 2, 3 * s // 2 - 1), (3 * s // 2 - 1, s // 2), (s, s)]
    variants = [(0.0, 0.5, 0.4, 0.6, False, False, None), (0.0, 1.5, 0.6, 0.4, True, False, (0.985, 0.3, 0.6)), (17.0, 1.0, 0.5, 0.5, False, True, (1.015, 1.7, 1.4)),
                (17.0, 0.5, 0.4, 0.4, True, True, (1.015, 0.3, 1.4)), (-17.0, 1.5, 0.6, 0.6, False, False, (0.985, 1.7, 0.6))]
    table = np.zeros(B, A.REC)
    for b in range(B):
        ang, sc, tx, ty, lr, ud, gains = variants[(b + seed) % 5]
        A.make_record(table[b], A.affine(S, s, ang, sc, tx, ty), sc, s, mosaic, centres[(b + seed) % 5], rng.randint(0, N, 4), lr, ud, gains)
    return table


def rect_row(cls, cx, cy, w, h, theta, s):
    """a label row as the tiler writes it: class + the corners of an oriented rectangle, clipped to the tile and normalised"""
    return np.concatenate([[cls], np.clip(xywhr_corners((cx, cy, w, h, theta)), 0, s).reshape(8) / s])


def label_pool(N, Lmax, s, seed, empty=(), counts=None):
    """counts: the number of rows per tile where the caller sets it (None or a negative entry: drawn from 1 .. Lmax)"""
    rng = np.random.RandomState(seed)
    lab, cnt = np.zeros((N, Lmax, 9)), np.zeros(N, np.int32)
    for t in range(N):
        if t in empty:
            continue
        cnt[t] = rng.randint(1, Lmax + 1) if counts is None or counts[t] < 0 else counts[t]
        for l in range(cnt[t]):
            lab[t, l] = rect_row(rng.randint(0, 12), rng.uniform(0, s), rng.uniform(0, s), rng.uniform(3, s / 2), rng.uniform(3, s / 2), rng.uniform(-1.5, 1.5), s)
    return lab, cnt


def label_cases():
    """[(name, s, pool_labels, pool_counts, table, n_cap)]: the label cases of the GPU suite.  The dedicated tie case (a square) is not in this list."""
    A = _aug()
    cases = []
    for seed, s, mosaic in ((1, 64, True), (2, 40, True), (3, 32, False), (4, 64, False)):
        lab, cnt = label_pool(7, 6, s, seed, empty=(3,))
        cfg = A.AugmentConfig(degrees=17.0) if seed % 2 else A.AugmentConfig()
        cfg = cfg if mosaic else cfg.close_mosaic()
        cases.append((f"seed{seed}-s{s}-{'mosaic' if mosaic else 'single'}", s, lab, cnt, A.sample_params(cfg, 5, 7, s, np.random.RandomState(100 + seed)), 24))
    s = 64
    # a label cut by the tile edge into a pentagon: a square turned by 45 degrees whose right corner the warp pushes out of the tile
    lab, cnt = np.zeros((1, 2, 9)), np.array([2], np.int32)
    lab[0, 0] = rect_row(5, 40, 30, 30, 22, math.pi / 4 + 0.1, s)
    lab[0, 1] = rect_row(7, 20, 50, 12, 6, 0.3, s)
    t = np.zeros(1, A.REC)
    A.make_record(t[0], A.affine(s, s, 0.0, 1.0, 0.5 + 12 / s, 0.5), 1.0, s)
    cases.append(("pentagon", s, lab, cnt, t, 4))
    # a label clipped to nothing: the translation moves it out of the tile altogether (the second one stays)
    lab2 = np.zeros((1, 2, 9))
    lab2[0, 0] = rect_row(1, 56, 30, 10, 8, 0.2, s)
    lab2[0, 1] = rect_row(2, 12, 30, 10, 8, 0.2, s)
    t2 = np.zeros(1, A.REC)
    A.make_record(t2[0], A.affine(s, s, 0.0, 1.0, 0.5 + 20 / s, 0.5), 1.0, s)
    cases.append(("clipped-away", s, lab2, cnt.copy(), t2, 4))
    # more survivors than n_cap
    lab3, cnt3 = label_pool(4, 8, s, 9)
    cases.append(("n_cap-2", s, lab3, cnt3, A.sample_params(A.AugmentConfig(scale=0.1), 3, 4, s, np.random.RandomState(77)), 2))
    # every source empty
    cases.append(("empty-pool", s, np.zeros((3, 4, 9)), np.zeros(3, np.int32), A.sample_params(A.AugmentConfig(), 2, 3, s, np.random.RandomState(5)), 3))
    return cases


# ---------------------------------------------------------------- the cases at the kernels' launch and domain edges
def centre_ends(s):
    """mosaic centres at the ends of what the kernels accept ([0, 2 s] each way): one or two quadrants of the canvas are empty"""
    return [(0, 0), (2 * s, 2 * s), (0, 2 * s), (2 * s, 0), (s, 0), (0, s), (2 * s, s)]


def centre_table(s, centre, src, hsv=True):
    """three mosaic records around one centre: scale 0.5 (all of the canvas in view), the identity scale with translation 0.5 (the canvas' middle),
    scale 0.5 flipped both ways"""
    A = _aug()
    t = np.zeros(3, A.REC)
    for b, (sc, flip, gains) in enumerate([(0.5, False, (1.015, 1.7, 1.4)), (1.0, False, (0.985, 0.3, 0.6)), (0.5, True, (1.0, 1.0, 1.0))]):
        A.make_record(t[b], A.affine(2 * s, s, 0.0, sc, 0.5, 0.5), sc, s, True, centre, src, flip, flip, gains if hsv else None)
    return t


OFF_BORDER = 3  # the first records of offcanvas_table leave the whole tile on the border value


def offcanvas_table(N, s, mosaic, hsv, seed):
    """maps that leave the canvas.  0: a translation by five tile sides; 1, 2: every `inv` entry +-1e7, written into the record (no matrix the
    sampler draws gives it): both fixed-point terms saturate at +-2^29 and their sum stays outside the canvas; 3: +-1e7 with opposite signs: the
    saturated terms cancel wherever x, y >= 1, so those pixels show canvas(0, 0) -- only with the saturation; the rest of row and column 0 stays outside"""
    A = _aug()
    rng = np.random.RandomState(seed)
    S, gains = (2 * s if mosaic else s), ((1.015, 1.7, 1.4) if hsv else None)
    t = np.zeros(4, A.REC)
    A.make_record(t[0], A.affine(S, s, 0.0, 1.0, 5.5, 0.5), 1.0, s, mosaic, (s, s), rng.randint(0, N, 4), False, False, gains)
    for b, inv in ((1, [1e7] * 6), (2, [-1e7] * 6), (3, [1e7, -1e7, 0.0, -1e7, 1e7, 0.0])):
        A.make_record(t[b], np.eye(3), 1.0, s, mosaic, (s, s), rng.randint(0, N, 4), False, b == 2, gains)
        t["inv"][b] = inv
    return t


def colour_pool():
    """all 2^24 colours as 16 tiles of side 1024, C = 3: colour c = t << 20 | y << 10 | x with b = c & 255, g = (c >> 8) & 255, r = c >> 16"""
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([c & 255, (c >> 8) & 255, c >> 16], -1).astype(np.uint8).reshape(16, 1024, 1024, 3)


HUE_LUT_OUT_OF_RANGE = "hue>=180"


def colour_table(gains, tiles=range(16)):
    """identity records (no mosaic) with the HSV bit set, one per tile of `colour_pool`.  gains = HUE_LUT_OUT_OF_RANGE: a hand-written table whose hue
    entries run from 76 to 255 over the hues 0 .. 179 (those of 104 and above are no hue: the sector falls outside 0 .. 5), unit saturation / value"""
    A = _aug()
    t = np.zeros(len(tiles), A.REC)
    for b, tile in enumerate(tiles):
        A.make_record(t[b], np.eye(3), 1.0, 1024, src=(tile, 0, 0, 0), hsv_gains=(1.0, 1.0, 1.0) if isinstance(gains, str) else gains)
        if isinstance(gains, str):
            t["lut"][b, :256] = np.minimum(76 + np.arange(256), 255)
    return t


def pass_survivors(lab, cnt, table, s):
    """per output tile, the survivors among the candidates [256 k, 256 k + 256), k = 0, 1, ..., in the label kernel's candidate order q * Lmax + l
    (it takes 256 candidates per pass of its prefix sum)"""
    Lmax, out = lab.shape[1], []
    for rec in table:
        nq = 4 if rec["flags"] & 1 else 1
        per = [0] * max(1, -(-nq * Lmax // 256))
        for q in range(nq):
            t = int(rec["src"][q])
            for l in range(min(max(int(cnt[t]), 0), Lmax)):
                per[(q * Lmax + l) // 256] += candidate_ref(rec, q, lab[t, l], s) is not None
        out.append(per)
    return out


def canvas_extent(rec, q, row, s):
    """-> (w, h, w0, h0): a label's axis-aligned extent on the mosaic canvas after and before the cut at the canvas"""
    padx, pady = float(rec["xc"] if q & 1 else rec["xc"] - s), float(rec["yc"] if q & 2 else rec["yc"] - s)
    P = np.asarray(row[1:], np.float64).reshape(4, 2) * s + [padx, pady]
    Q = np.clip(P, 0.0, 2.0 * s)
    return (np.ptp(Q[:, 0]), np.ptp(Q[:, 1]), np.ptp(P[:, 0]), np.ptp(P[:, 1]))


EDGE_LMAX = ((65, "fits", 0), (100, "inside", 0), (256, "boundary", 0))  # (Lmax, where n_cap falls, seed): re-seeded until the margins hold
EDGE_SEEDS = {"n_cap": 0, "counts": 0, "centre": 0}
CENTRE_EXTRA = lambda s: (s // 4, 2 * s - s // 4)  # (not an end: here the canvas cuts labels in part)


def _lmax_case(Lmax, mode, seed, s=64):
    A = _aug()
    lab, cnt = label_pool(5, Lmax, s, 300 + seed, empty=(1,), counts=[Lmax, 0, Lmax - 1, -1, -1])
    table = A.sample_params(A.AugmentConfig(scale=0.1), 3, 5, s, np.random.RandomState(400 + seed), [0, 2, 3])
    table["src"][0] = (0, 2, 3, 0)  # the full tile in the last quadrant too: the candidates run up to 4 Lmax - 1
    table["src"][1] = (2, 1, 0, 0)  # the empty tile in the middle of the candidate list
    per = pass_survivors(lab, cnt, table, s)
    if mode == "fits":
        n_cap = max(sum(p) for p in per) + 3
    elif mode == "inside":  # n_cap is reached inside the second pass of the tile with the most survivors in both of its first two
        p = max(per, key=lambda p: min(p[0], p[1]))
        n_cap = p[0] + max(p[1] // 2, 1)
    else:  # n_cap = the survivors of the first pass of the tile with the most survivors behind it
        n_cap = max(per, key=lambda p: sum(p[1:]))[0]
    return f"Lmax{Lmax}-{mode}", s, lab, cnt, table, n_cap


@functools.lru_cache(maxsize=None)
def label_edge_cases():
    """[(name, s, pool_labels, pool_counts, table, n_cap)] like label_cases(): several passes of the label kernel's prefix sum, n_cap reached in a later
    pass and at a pass boundary, a zero-fill that strides, pool counts outside [0, Lmax], Lmax = 0, mosaic centres at the ends.  All at s = 64.
    Built once per process; nobody writes into them."""
    A = _aug()
    s, cases = 64, [_lmax_case(L, mode, seed) for L, mode, seed in EDGE_LMAX]
    lab, cnt = label_pool(7, 6, s, 500 + EDGE_SEEDS["n_cap"], empty=(3,))
    table = A.sample_params(A.AugmentConfig(), 3, 7, s, np.random.RandomState(510 + EDGE_SEEDS["n_cap"]))
    cases += [(f"few-n_cap{n}", s, lab, cnt, table, n) for n in (1, 257, 600)]
    lab, cnt = label_pool(5, 6, s, 520 + EDGE_SEEDS["counts"], counts=[6] * 5)
    cnt[1], cnt[3] = 6 + 5, -3  # every row of both tiles holds a label: the first must give 6 candidates, the second none
    table = A.sample_params(A.AugmentConfig(scale=0.1), 3, 5, s, np.random.RandomState(530 + EDGE_SEEDS["counts"]))
    table["src"][0], table["src"][1] = (1, 3, 0, 2), (1, 1, 3, 1)
    cases.append(("counts-outside", s, lab, cnt, table, 40))
    cases.append(("Lmax0", s, np.zeros((3, 0, 9)), np.array([0, 3, -1], np.int32), A.sample_params(A.AugmentConfig(), 2, 3, s, np.random.RandomState(540)), 5))
    for k, centre in enumerate(centre_ends(s) + [CENTRE_EXTRA(s)]):
        lab, cnt = label_pool(4, 6, s, 550 + 10 * EDGE_SEEDS["centre"] + k, counts=[6] * 4)
        cases.append((f"centre-{centre[0]}-{centre[1]}", s, lab, cnt, centre_table(s, centre, (0, 1, 2, 3)), 24))
    return cases
