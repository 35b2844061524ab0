"""Exact rational reference for the quad geometry (polygon IoU, validity, point-in-quad) and the two decision loops built on it.

Pure Python, `fractions.Fraction` throughout; the inputs are the doubles the kernels receive, converted exactly.  Nothing here is shared
with oracle/ or csrc/: no envelope test, no Sutherland-Hodgman on the quads themselves, no early exit -- both quads are cut into triangles
and the intersection is the sum of four exact triangle-triangle areas.

  valid(quad)                          the project's restatement of polygon validity (see the docstring: parity with GEOS is NOT claimed)
  iou(a, b)                            -> (Fraction, nearest double)
  point_strictly_inside(quad, x, y)    exact crossing number, boundary excluded
  iou_bound(a, b)                      a-priori bound on |fp64 evaluation - exact|
  greedy_merge / consensus             the reference's loops over exact IoU, with the count of pairs the fp64 evaluation cannot decide
"""
import functools
import math
from fractions import Fraction as F

U = 2.0 ** -53  # fp64 unit roundoff


# ------------------------------------------------------------------------------------------------ basics
def _finite(quad):
    return all(math.isfinite(float(v)) for v in quad[:8])


def _pts(quad):
    return [(F(float(quad[2 * i])), F(float(quad[2 * i + 1]))) for i in range(4)]


def _cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _area2(P):
    return sum(P[i][0] * P[(i + 1) % len(P)][1] - P[(i + 1) % len(P)][0] * P[i][1] for i in range(len(P)))


def _between(a, b, c):
    """c is known to be collinear with a, b: does it lie on the closed segment ab?"""
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def _segments_share_a_point(a, b, c, d):
    d1, d2, d3, d4 = _cross(a, b, c), _cross(a, b, d), _cross(c, d, a), _cross(c, d, b)
    if ((d1 > 0 and d2 < 0) or (d1 < 0 and d2 > 0)) and ((d3 > 0 and d4 < 0) or (d3 < 0 and d4 > 0)):
        return True
    return ((d1 == 0 and _between(a, b, c)) or (d2 == 0 and _between(a, b, d)) or (d3 == 0 and _between(c, d, a)) or (d4 == 0 and _between(c, d, b)))


def valid(quad):
    """The project's restatement of GEOS polygon validity for a ring of four vertices (GEOS cannot be consulted here: this is the rule the
    project states, not a claim of parity with it).  A quad is valid iff
      * all eight coordinates are finite,
      * its signed area is not zero,
      * no two non-adjacent edges share a point,
      * no two adjacent edges fold back onto each other (a spike: the vertex between them is collinear with its neighbours and both lie on
        the same side of it).
    A vertex that lies straight through between its neighbours is allowed, and so is a vertex repeated consecutively (the ring is then a
    triangle: the repeated vertex is dropped before the rules above are applied, and a triangle of non-zero area satisfies all of them)."""
    if not _finite(quad):
        return False
    P = _pts(quad)
    if _area2(P) == 0:
        return False
    R = [P[i] for i in range(4) if P[i] != P[i - 1]]  # repeated consecutive vertices dropped (cyclically)
    if len(R) < 4:
        return len(R) == 3  # a triangle of non-zero area
    if _segments_share_a_point(P[0], P[1], P[2], P[3]) or _segments_share_a_point(P[1], P[2], P[3], P[0]):
        return False
    for i in range(4):
        a, b, c = P[i - 1], P[i], P[(i + 1) % 4]
        if _cross(a, b, c) == 0 and (a[0] - b[0]) * (c[0] - b[0]) + (a[1] - b[1]) * (c[1] - b[1]) > 0:
            return False
    return True


def point_strictly_inside(quad, x, y):
    """1 iff the quad is valid and (x, y) lies in its interior: exact crossing number of the ray to +x; a point on the boundary is outside."""
    if not (math.isfinite(float(x)) and math.isfinite(float(y))) or not valid(quad):
        return 0
    P = _pts(quad)
    q = (F(float(x)), F(float(y)))
    crossings = 0
    for i in range(4):
        a, b = P[i], P[(i + 1) % 4]
        if a == b:
            if q == a:
                return 0
            continue
        if _cross(a, b, q) == 0 and _between(a, b, q):
            return 0
        if (a[1] > q[1]) != (b[1] > q[1]):  # the edge spans the ray's line (half-open in y)
            xi = a[0] + (q[1] - a[1]) * (b[0] - a[0]) / (b[1] - a[1])
            if xi > q[0]:
                crossings += 1
    return crossings & 1


# ------------------------------------------------------------------------------------------------ exact IoU
def _ccw(P):
    return P if _area2(P) > 0 else P[::-1]


def _fan(P, s):
    return [(P[s], P[(s + 1) % 4], P[(s + 2) % 4]), (P[s], P[(s + 2) % 4], P[(s + 3) % 4])]


def _reflex(P):
    """index of the reflex vertex of a counter-clockwise simple quad, or None"""
    for i in range(4):
        if _cross(P[i - 1], P[i], P[(i + 1) % 4]) < 0:
            return i
    return None


def _tri_tri_area2(S, T):
    """twice the area of the intersection of two counter-clockwise triangles with INTEGER vertices (zero-area triangles contribute
    nothing): the subject is cut by the three half-planes of the other.  A cut vertex is the exact rational point, held in homogeneous
    integers (x / w, y / w), w > 0 -- the same numbers as Fractions, without a gcd per operation; the area is summed as Fractions."""
    if _area2(list(S)) == 0 or _area2(list(T)) == 0:
        return F(0)
    poly = [(x, y, 1) for (x, y) in S]
    for e in range(3):
        (ax, ay), (bx, by) = T[e], T[(e + 1) % 3]
        dx, dy = bx - ax, by - ay
        D = [dx * (y - ay * w) - dy * (x - ax * w) for (x, y, w) in poly]  # w * cross(a, b, p): its sign is the side of p
        out = []
        for i in range(len(poly)):
            s, p, ds, dp = poly[i - 1], poly[i], D[i - 1], D[i]
            if (ds < 0) != (dp < 0):  # s + (p - s) ds / (ds - dp)
                x, y, w = p[0] * ds - s[0] * dp, p[1] * ds - s[1] * dp, p[2] * ds - s[2] * dp
                g = math.gcd(x, y, w)
                if w < 0:
                    g = -g
                out.append((x // g, y // g, w // g))
            if dp >= 0:
                out.append(p)
        poly = out
        if not poly:
            return F(0)
    return abs(sum(F(poly[i - 1][0] * poly[i][1] - poly[i][0] * poly[i - 1][1], poly[i - 1][2] * poly[i][2]) for i in range(len(poly))))


def _inter2(Ta, Tb):
    return sum(_tri_tri_area2(s, t) for s in Ta for t in Tb)


def areas(a, b):
    """exact (area a, area b, intersection) of two VALID quads"""
    tx, ty = math.floor(float(a[0])), math.floor(float(a[1]))  # areas are invariant under an exact (rational) translation: one cache entry per shape
    return _areas(tuple(F(float(c)) - (tx if k % 2 == 0 else ty) for k, c in enumerate(list(a[:8]) + list(b[:8]))))


@functools.lru_cache(maxsize=65536)
def _areas(key):
    P, Q = [(key[2 * i], key[2 * i + 1]) for i in range(4)], [(key[8 + 2 * i], key[9 + 2 * i]) for i in range(4)]
    scale = max(c.denominator for pt in P + Q for c in pt)  # doubles are dyadic: one power of two makes all sixteen integers
    P, Q = _ccw([(int(x * scale), int(y * scale)) for x, y in P]), _ccw([(int(x * scale), int(y * scale)) for x, y in Q])
    rp, rq = _reflex(P), _reflex(Q)
    inter2 = _inter2(_fan(P, rp if rp is not None else 0), _fan(Q, rq if rq is not None else 0))
    if rp is None or rq is None:  # self-check: the other diagonal of a convex operand gives the same intersection
        other = _inter2(_fan(P, rp if rp is not None else 1), _fan(Q, rq if rq is not None else 1))
        assert other == inter2, "triangulations disagree"
    return F(abs(_area2(P)), 2 * scale * scale), F(abs(_area2(Q)), 2 * scale * scale), inter2 / (2 * scale * scale)


def iou(a, b):
    """-> (exact IoU as a Fraction, its nearest double).  An invalid operand gives 0.  No envelope test, no early exit."""
    if not valid(a) or not valid(b):
        return F(0), 0.0
    a1, a2, inter = areas(a, b)
    v = inter / (a1 + a2 - inter)
    return v, v.numerator / v.denominator  # int / int is correctly rounded


# ------------------------------------------------------------------------------------------------ the a-priori error bound
EXACT_SIDE = 16  # n * (k / n) == k in fp64 for all 0 <= k <= n <= EXACT_SIDE (enumerated in test_geom_exact_cpu.py; it first fails at 22 * (15 / 22))


def _int_axis_rect(quad):
    v = [float(c) for c in quad[:8]]
    if any(c != math.floor(c) or abs(c) >= 2.0 ** 20 for c in v):
        return False
    xs, ys = sorted(set(v[0::2])), sorted(set(v[1::2]))
    if len(xs) != 2 or len(ys) != 2 or xs[1] - xs[0] > EXACT_SIDE or ys[1] - ys[0] > EXACT_SIDE:
        return False
    return all((v[2 * i] == v[2 * ((i + 1) % 4)]) != (v[2 * i + 1] == v[2 * ((i + 1) % 4) + 1]) for i in range(4))  # every edge axis-parallel


def iou_bound(a, b, exact=None):
    """The largest |device - exact| that a correct fp64 evaluation of clip_area / shoelace2 / the final division can show, as a function of
    M (largest |coordinate|), the extents of the two quads, the two areas and the union.  u = 2^-53; e_a, e_b = diagonals of the two
    envelopes, E = e_a + e_b (any two points the clip touches are closer than E), d = min(e_a, e_b) (the intersection lies inside both, so
    every chord of it is shorter than d).

    cross3(a, b, p): the four differences are rounded RELATIVE to themselves (no M), the two products and the subtraction likewise:
        |d cross| <= 8 u L E,  L = |ab| the clip edge.  A wrong sign therefore needs p within 8 u E of the clip line, and deciding such a
        point the other way moves the cut by as much: area change <= 8 u E d per chord, two chords (entering, leaving) per clip edge.
    interpolation t = ds / (ds - dp), v = s + (p - s) t: ds and dp have opposite signs, so |dt| <= 16 u L E / |ds - dp| + 2 u; the point
        slides ALONG the subject edge by |p - s| dt, which changes the area by half that times the distance of the neighbouring vertex
        from the subject edge's line (<= d sin(angle)): the angle cancels and <= 9 u E d is left per new vertex, two per clip edge.
        The rounding of (p - s), of the product and of the sum at magnitude M displaces v by at most u M + 2 u E per coordinate: area
        change <= (u M + 2 u E) d per vertex, taken twice for its passage through the later clip edges, 8 vertices at most.
        Four clip edges:  d_clip = u d (4 (16 + 18) E + 16 (M + 2 E)) = u d (168 E + 16 M).
    shoelace2 over n vertices on ABSOLUTE coordinates: each product x_i y_j is rounded at magnitude M^2 (u M^2 each, two per term); a
        term's exact value is <= 2 M d, so the subtraction and the n additions add u (n + n^2) 2 M d:  d_shoe(n, d) = u (n M^2 + (n + n^2) M d)
        on the area (half the sum).  n = 4 for the operands (d = their own extent), n <= 8 for a clipped convex quad.
    d_inter = d_clip + d_shoe(8, d) when an operand is convex; the concave x concave path sums four triangle clips:
        4 (d_clip + d_shoe(6, d)) + 4 u inter.
    union = a1 + a2 - inter: d_union = d_a1 + d_a2 + d_inter + 3 u (a1 + a2).
    division: (I + dI) / (U - dU) - I / U = (dI + iou dU) / (U - dU), plus the division's own rounding u iou.  If dU >= U the bound is 1.

    The shoelace and division terms are rigorous and dominate wherever M is large; the two clip terms are first-order estimates (slivers,
    each displaced vertex counted twice), generous in their constants rather than proven.  Measured, the worst |fp64 - exact| is 0.26 of
    this bound over the families below.

    Exactly representable case: two axis-parallel rectangles with integer coordinates below 2^20 and sides of at most EXACT_SIDE.  Every
    difference, product and sum above is then an integer below 2^53, t = fl(k / n) for integers 0 <= k <= n <= EXACT_SIDE and
    fl(n t) = k (enumerated), so every intermediate is exact and only the final division rounds -- correctly: the bound is
    |nearest double of the exact IoU - exact IoU|, which is 0 for a dyadic IoU.  (For other integer quads the quotient t is NOT exact --
    a diamond's edge cut at a third -- so they get the general bound; with integer operands d_a1 = d_a2 = 0, as their shoelace is exact.)"""
    if not valid(a) or not valid(b):
        return 0.0
    ex, exd = exact if exact is not None else iou(a, b)
    if _int_axis_rect(a) and _int_axis_rect(b):
        return float(abs(F(exd) - ex))
    va, vb = [float(c) for c in a[:8]], [float(c) for c in b[:8]]
    M = max(abs(c) for c in va + vb)
    ea = math.hypot(max(va[0::2]) - min(va[0::2]), max(va[1::2]) - min(va[1::2]))
    eb = math.hypot(max(vb[0::2]) - min(vb[0::2]), max(vb[1::2]) - min(vb[1::2]))
    E, d = ea + eb, min(ea, eb)
    a1, a2, inter = (float(v) for v in areas(a, b))
    ints = all(c == math.floor(c) and abs(c) < 2.0 ** 20 for c in va + vb)
    shoe = lambda n, ext: U * (n * M * M + (n + n * n) * M * ext)
    d_a1, d_a2 = (0.0, 0.0) if ints else (shoe(4, ea), shoe(4, eb))
    d_clip = U * d * (168.0 * E + 16.0 * M)
    both_concave = _reflex(_ccw(_pts(a))) is not None and _reflex(_ccw(_pts(b))) is not None
    d_inter = 4.0 * (d_clip + shoe(6, d)) + 4.0 * U * inter if both_concave else d_clip + shoe(8, d)
    uni = a1 + a2 - inter
    d_uni = d_a1 + d_a2 + d_inter + 3.0 * U * (a1 + a2)
    if d_uni >= uni:
        return 1.0
    return min(1.0, (d_inter + float(ex) * d_uni) / (uni - d_uni) + U * float(ex))


def cannot_decide(exact, thr, bound):
    """Could a value within `bound` of `exact` fall on the other side of `>= thr`?  (|exact - thr| <= bound, except that an exact tie with a
    bound of exactly 0 IS decided: the evaluation reproduces the tie.)"""
    if float(thr) <= 0.0:
        return False  # neither evaluation is ever negative
    thr = F(float(thr))
    return (exact - F(bound) < thr) if exact >= thr else (exact + F(bound) >= thr)


# ------------------------------------------------------------------------------------------------ decisions over exact IoU
def _envelope(q):
    v = [float(c) for c in q[:8]]
    return min(v[0::2]), min(v[1::2]), max(v[0::2]), max(v[1::2])


class PairIoU:
    """exact IoU of rows of one box array, cached per unordered pair.  The only pair skip is an exact one: two envelopes that are strictly
    disjoint, compared on the input doubles, cannot intersect (IoU 0) -- an invalid quad's IoU is 0 anyway."""

    def __init__(self, boxes):
        self.boxes = [[float(c) for c in b[:8]] for b in boxes]
        self.env = [_envelope(b) if _finite(b) else None for b in self.boxes]
        self.cache, self.shapes = {}, {}

    def neighbours(self):
        """row -> rows whose envelope is not strictly disjoint from its own (the same exact comparison, vectorised)"""
        import numpy as np
        ok = np.array([e is not None for e in self.env])
        E = np.array([e if e is not None else (1.0, 1.0, -1.0, -1.0) for e in self.env])
        out = []
        for i in range(len(E)):
            hit = ok & ok[i] & ~((E[:, 2] < E[i, 0]) | (E[i, 2] < E[:, 0]) | (E[:, 3] < E[i, 1]) | (E[i, 3] < E[:, 1]))
            hit[i] = False
            out.append(np.nonzero(hit)[0].tolist())
        return out

    def __call__(self, i, j):
        key = (i, j) if i < j else (j, i)
        if key not in self.cache:
            ei, ej = self.env[i], self.env[j]
            if ei is None or ej is None or ei[2] < ej[0] or ej[2] < ei[0] or ei[3] < ej[1] or ej[3] < ei[1]:
                self.cache[key] = (F(0), 0.0)
            else:
                a, b = self.boxes[key[0]], self.boxes[key[1]]
                # two exactly evaluated integer rectangles: IoU and bound depend on the shape of the pair alone, not on where it lies
                shape = tuple(c - a[n % 2] for n, c in enumerate(a + b)) if _int_axis_rect(a) and _int_axis_rect(b) else None
                if shape is None or shape not in self.shapes:
                    ex = iou(a, b)
                    val = (ex[0], iou_bound(a, b, ex))
                    if shape is not None:
                        self.shapes[shape] = val
                else:
                    val = self.shapes[shape]
                self.cache[key] = val
        return self.cache[key]


def _stable_desc(conf):
    return sorted(range(len(conf)), key=lambda i: -float(conf[i]))  # sorted() is stable: ties keep input order


def greedy_merge(boxes, cls, conf, thr, pair=None):
    """merge_detections (Detect_OBB.py:176-200) over exact IoU: stable sort by confidence descending, a detection is kept unless a kept
    one of its class has IoU >= thr with it.  -> ((order, keep flags in sorted order), undecided).  `undecided` counts the evaluated
    pairs whose exact IoU is too close to thr for an fp64 evaluation to decide (cannot_decide).  The only pair skip permitted is the exact
    one of PairIoU: a strictly disjoint envelope comparison on the input doubles."""
    pair = pair or PairIoU(boxes)
    order = _stable_desc(conf)
    nbr, rank = pair.neighbours(), {}
    keep, undecided, seen = [], 0, set()
    thr_pos = float(thr) > 0.0
    for di in order:
        k = 1
        # kept rows in the order they were kept; with thr > 0 only those the exact envelope comparison leaves (the others have IoU 0 < thr)
        for dj in (sorted((d for d in nbr[di] if d in rank), key=rank.get) if thr_pos else sorted(rank, key=rank.get)):
            if int(cls[di]) != int(cls[dj]):
                continue
            ex, bound = pair(di, dj)
            if (di, dj) not in seen:
                seen.add((di, dj))
                undecided += cannot_decide(ex, thr, bound)
            if ex >= F(float(thr)):
                k = 0
                break
        keep.append(k)
        if k:
            rank[di] = len(rank)
    return (order, keep), undecided


def consensus(boxes, cls, conf, offsets, iou_partner=0.40, cons_low=0.25, cons_high=0.70, pair=None):
    """cross_scale_consensus_filter (Detect_OBB.py:347-423) over exact IoU.  Scale s owns rows [offsets[s], offsets[s + 1]).
    -> (kept row indices in output order, undecided).  `undecided` counts the evaluated pairs whose IoU cannot be decided against
    iou_partner, plus the pairs of candidates of one detection with equal confidence whose IoUs (the tie-break) are closer than their
    bounds.  The only pair skip permitted is the exact one of PairIoU: a strictly disjoint envelope comparison on the input doubles."""
    pair = pair or PairIoU(boxes)
    ns, total = len(offsets) - 1, offsets[-1]
    if ns == 1:
        return list(range(total)), 0
    alive = [float(conf[i]) >= cons_low for i in range(total)]
    visited = [False] * total
    out, undecided = [], 0
    thr = F(float(iou_partner))
    for s in range(ns):
        for i in range(offsets[s], offsets[s + 1]):
            if not alive[i] or visited[i]:
                continue
            best, cands = None, []
            for t in range(ns):
                if t == s:
                    continue
                for j in range(offsets[t], offsets[t + 1]):
                    if not alive[j] or visited[j] or int(cls[j]) != int(cls[i]):
                        continue
                    ex, bound = pair(i, j)
                    undecided += cannot_decide(ex, iou_partner, bound)
                    if ex >= thr:
                        cands.append((j, ex, bound))
                        cp = float(conf[j])
                        if best is None or cp > best[1] or (cp == best[1] and ex > best[2]):
                            best = (j, cp, ex)
            if best is not None:  # the tie-break on IoU among candidates of the best confidence
                top = [c for c in cands if float(conf[c[0]]) == best[1]]
                for x in range(len(top)):
                    for y in range(x + 1, len(top)):
                        if top[x][1] != top[y][1] and abs(top[x][1] - top[y][1]) <= F(top[x][2]) + F(top[y][2]):
                            undecided += 1
                        if top[x][1] == top[y][1] and (top[x][2] > 0 or top[y][2] > 0):
                            undecided += 1
            if best is None or best[1] < cons_low:
                if float(conf[i]) >= cons_high:
                    out.append(i)
                visited[i] = True
                continue
            out.append(i if float(conf[i]) >= best[1] else best[0])
            visited[i] = True
            visited[best[0]] = True
    return out, undecided


# ------------------------------------------------------------------------------------------------ test populations (shared by the CPU and GPU tests)
def rect(cx, cy, w, h, r=0.0):
    c, s = math.cos(r), math.sin(r)
    v1, v2 = (w / 2 * c, w / 2 * s), (-h / 2 * s, h / 2 * c)
    return [cx + v1[0] + v2[0], cy + v1[1] + v2[1], cx + v1[0] - v2[0], cy + v1[1] - v2[1],
            cx - v1[0] - v2[0], cy - v1[1] - v2[1], cx - v1[0] + v2[0], cy - v1[1] + v2[1]]


def box(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def relabel(q, start, reverse):
    p = [(q[2 * i], q[2 * i + 1]) for i in range(4)]
    if reverse:
        p = p[::-1]
    p = p[start:] + p[:start]
    return [c for pt in p for c in pt]


def _arrow(rng, integer=False):
    """a concave (arrow-head) quad: tip, wing, notch, wing; the notch is the reflex vertex"""
    if integer:
        x, y, w, h, n = (int(v) for v in (rng.integers(0, 12), rng.integers(0, 12), rng.integers(3, 9), rng.integers(2, 6), 0))
        n = int(rng.integers(1, w))
        q = [x, y, x + w, y + h, x, y + 2 * h, x + n, y + h]
    else:
        x, y, w, h = rng.uniform(0, 30), rng.uniform(0, 30), rng.uniform(10, 40), rng.uniform(5, 20)
        n = rng.uniform(0.1, 0.9) * w
        q = [x, y, x + w, y + h, x, y + 2 * h, x + n, y + h]
        r = rng.uniform(0, 2 * math.pi)
        c, s = math.cos(r), math.sin(r)
        q = [v for i in range(4) for v in (c * q[2 * i] - s * q[2 * i + 1], s * q[2 * i] + c * q[2 * i + 1])]
    return relabel(q, int(rng.integers(0, 4)), bool(rng.integers(0, 2)))


def _f32(v):
    import numpy as np
    return float(np.float32(v))


def _make_family(name):
    import numpy as np
    rng = np.random.default_rng({"a": 11, "b": 12, "c": 13, "d": 14, "e": 15, "f": 16, "g": 17}[name])
    A, B = [], []
    if name == "a":  # integer axis-parallel rectangles on the 0..11 lattice, every cyclic start and both windings
        for n in range(640):
            xa, ya, xb, yb = (sorted(rng.choice(12, 2, replace=False).tolist()) for _ in range(4))
            if n % 10 == 0:
                xb, yb = xa, ya  # equal boxes
            if n % 10 == 1:
                xb, yb = [xa[1], xa[1] + 3], ya  # a shared edge
            if n % 10 == 2:
                xb, yb = [xa[1], xa[1] + 2], [ya[1], ya[1] + 2]  # a shared corner
            A.append(relabel(box(xa[0], ya[0], xa[1], ya[1]), n % 4, (n // 4) % 2 == 1))
            B.append(relabel(box(xb[0], yb[0], xb[1], yb[1]), (n // 8) % 4, (n // 32) % 2 == 1))
    elif name == "b":  # integer diamonds x squares
        for n in range(400):
            cx, cy, r = int(rng.integers(2, 10)), int(rng.integers(2, 10)), int(rng.integers(1, 6))
            x0, y0, s = int(rng.integers(0, 10)), int(rng.integers(0, 10)), int(rng.integers(1, 8))
            if n % 8 == 0:
                x0, y0 = cx + r, cy - s // 2  # the diamond's right tip touches the square's left edge
            A.append(relabel([cx + r, cy, cx, cy + r, cx - r, cy, cx, cy - r], n % 4, (n // 4) % 2 == 1))
            B.append(box(x0, y0, x0 + s, y0 + s))
            if n % 2:
                A[-1], B[-1] = B[-1], A[-1]
    elif name == "c":  # random rotated rectangles at three offsets
        for off in (0.0, 4096.0, 65536.0):
            for _ in range(300):
                A.append(rect(off + rng.uniform(0, 50), off + rng.uniform(0, 50), rng.uniform(5, 40), rng.uniform(5, 40), rng.uniform(0, math.pi)))
                B.append(rect(off + rng.uniform(0, 50), off + rng.uniform(0, 50), rng.uniform(5, 40), rng.uniform(5, 40), rng.uniform(0, math.pi)))
    elif name == "d":  # as the pipeline makes them: float32 local corners + an integer tile offset
        for _ in range(600):
            ox, oy = int(rng.integers(0, 65537)), int(rng.integers(0, 65537))
            for L in (A, B):
                q = rect(rng.uniform(100, 160), rng.uniform(100, 160), rng.uniform(8, 60), rng.uniform(8, 60), rng.uniform(0, math.pi))
                L.append([_f32(q[k]) + (ox if k % 2 == 0 else oy) for k in range(8)])
    elif name == "e":  # concave x concave, concave x rectangle, integer concave
        for n in range(900):
            kind = n % 3
            if kind == 0:
                A.append(_arrow(rng)), B.append(_arrow(rng))
            elif kind == 1:
                A.append(_arrow(rng)), B.append(rect(rng.uniform(0, 40), rng.uniform(0, 40), rng.uniform(5, 40), rng.uniform(5, 40), rng.uniform(0, math.pi)))
                if n % 2:
                    A[-1], B[-1] = B[-1], A[-1]
            else:
                A.append(_arrow(rng, integer=True)), B.append(_arrow(rng, integer=True))
    elif name == "f":  # rectangles 0.5 .. 3 px wide
        for n in range(400):
            off = (0.0, 4096.0, 65536.0)[n % 3]
            cx, cy, r = off + rng.uniform(0, 30), off + rng.uniform(0, 30), rng.uniform(0, math.pi)
            A.append(rect(cx, cy, rng.uniform(0.5, 3.0), rng.uniform(20, 80), r))
            B.append(rect(cx + rng.normal(0, 1.0), cy + rng.normal(0, 1.0), rng.uniform(0.5, 3.0), rng.uniform(20, 80), r + rng.normal(0, 0.05)))
    elif name == "g":  # one map-sized box against small ones
        big = rect(32768.0, 32768.0, 60000.0, 50000.0, 0.3)
        for n in range(300):
            ang = rng.uniform(0, 2 * math.pi)
            t = rng.uniform(0.8, 1.2) if n % 2 else rng.uniform(0, 0.9)  # half of them near the big box's boundary
            cx, cy = 32768.0 + t * 25000.0 * math.cos(ang), 32768.0 + t * 25000.0 * math.sin(ang)
            A.append(big if n % 4 < 2 else rect(cx, cy, rng.uniform(5, 60), rng.uniform(5, 60), rng.uniform(0, math.pi)))
            B.append(rect(cx, cy, rng.uniform(5, 60), rng.uniform(5, 60), rng.uniform(0, math.pi)) if n % 4 < 2 else big)
    return A, B


FAMILIES = ("a", "b", "c", "d", "e", "f", "g")
ZERO_TOLERANCE = ("a", "b")  # integer inputs whose every intermediate is representable: the fp64 evaluation must give the nearest double
# the code paths a family is there to reach (a family whose population of one of them is zero fails)
INTENDED = {"a": ("convex_convex", "contact_only"), "b": ("convex_convex", "contact_only", "envelope_only"), "c": ("convex_convex", "envelope_only"),
            "d": ("convex_convex", "envelope_only"), "e": ("one_concave", "both_concave", "envelope_only"), "f": ("convex_convex",), "g": ("convex_convex", "envelope_only")}


def _touch(a, b):
    P, Q = _pts(a), _pts(b)
    return any(_segments_share_a_point(P[i], P[(i + 1) % 4], Q[j], Q[(j + 1) % 4]) for i in range(4) for j in range(4))


@functools.lru_cache(maxsize=None)
def family(name):
    """-> dict(A, B [n][8], exact [n] Fractions, nearest [n] doubles, bound [n], tol [n] (0 for the ZERO_TOLERANCE families), pop: path -> count).
    Computed once per process and shared; callers must not modify it."""
    A, B = _make_family(name)
    exact, nearest, bound = [], [], []
    pop = {"convex_convex": 0, "one_concave": 0, "both_concave": 0, "envelope_only": 0, "contact_only": 0}
    for a, b in zip(A, B):
        assert valid(a) and valid(b)
        ex = iou(a, b)
        exact.append(ex[0]), nearest.append(ex[1]), bound.append(iou_bound(a, b, ex))
        nconc = (_reflex(_ccw(_pts(a))) is not None) + (_reflex(_ccw(_pts(b))) is not None)
        pop[("convex_convex", "one_concave", "both_concave")[nconc]] += 1
        ea, eb = _envelope(a), _envelope(b)
        if ex[0] == 0 and not (ea[2] < eb[0] or eb[2] < ea[0] or ea[3] < eb[1] or eb[3] < ea[1]):
            pop["contact_only" if _touch(a, b) else "envelope_only"] += 1
    tol = [0.0] * len(A) if name in ZERO_TOLERANCE else bound
    return {"A": A, "B": B, "exact": exact, "nearest": nearest, "bound": bound, "tol": tol, "pop": pop}


def check_family(name, got, what):
    """|got - exact| <= tol per pair (compared as exact rationals); prints the populations and the worst |err| / iou_bound; -> that ratio"""
    fam = family(name)
    worst, worst_abs = 0.0, 0.0
    for k, g in enumerate(got):
        err = abs(F(float(g)) - fam["exact"][k])
        if name in ZERO_TOLERANCE:
            assert float(g) == fam["nearest"][k], f"{what} family {name} pair {k}: got {float(g)!r}, the exact IoU rounds to {fam['nearest'][k]!r}"
        else:
            assert err <= F(fam["tol"][k]), f"{what} family {name} pair {k}: got {float(g)!r}, exact {float(fam['exact'][k])!r}, bound {fam['tol'][k]:.3e}"
        worst_abs = max(worst_abs, float(err))
        if err and name not in ZERO_TOLERANCE:
            worst = max(worst, float(err) / fam["bound"][k] if fam["bound"][k] else float("inf"))
    bs = sorted(fam["bound"])
    print(f"  {what} family {name}: {len(got)} pairs, populations {fam['pop']}, worst |err| = {worst_abs:.3e}, worst |err| / iou_bound = {worst:.4f}, "
          f"median iou_bound = {bs[len(bs) // 2]:.3e}")
    for path in INTENDED[name]:
        assert fam["pop"][path] > 0, f"family {name} never reaches {path}"
    return worst


# validity / point-in-quad table: small dyadic coordinates, so that every cross product of the fp64 evaluation is exact
TABLE_QUADS = {
    "square": box(0, 0, 4, 4), "square_cw": relabel(box(0, 0, 4, 4), 1, True), "diamond": [2, 0, 4, 2, 2, 4, 0, 2], "sheared": [0, 0, 4, 4, 4, 8, 0, 4],
    "arrow": [0, 0, 4, 2, 0, 4, 2, 2], "collinear_vertex": [0, 0, 2, 0, 4, 0, 2, 4], "spike": [0, 0, 4, 0, 2, 0, 2, 4], "bow_tie": [0, 0, 4, 4, 4, 0, 0, 4],
    "repeated_first": [0, 0, 0, 0, 4, 0, 0, 4], "repeated_mid": [0, 0, 4, 0, 4, 0, 0, 4], "repeated_wrap": [0, 0, 4, 0, 0, 4, 0, 0],
    "repeated_opposite": [0, 0, 4, 0, 0, 0, 0, 4], "vertex_on_edge": [0, 0, 4, 0, 4, 4, 2, 0], "line": [0, 0, 1, 1, 2, 2, 3, 3], "point": [1, 1, 1, 1, 1, 1, 1, 1],
    "nan": [0, 0, 4, 0, float("nan"), 4, 0, 4], "inf": [0, 0, 4, 0, float("inf"), 4, 0, 4], "square_far": box(65536, 65536, 65540, 65540),
    "diamond_far": [65538, 65536, 65540, 65538, 65538, 65540, 65536, 65538],
}


def table_hull(name):
    """a box around the table quad `name`: IoU against it pins the VALUE a valid table quad gives, not only that it is non-zero"""
    return box(65528, 65528, 65552, 65552) if "far" in name else box(-8, -8, 16, 16)


def table_points():
    """vertices, edge points, inside and outside points on a half-integer grid (every cross product exact in fp64), non-finite points, and the
    same grid moved to the far quads"""
    pts = [(i / 2, j / 2) for i in range(-1, 10) for j in range(-1, 18)]
    far = [(65536 + x, 65536 + y) for (x, y) in pts[::3]]
    return pts + far + [(float("nan"), 1.0), (1.0, float("inf")), (float("-inf"), 2.0)]


def table_ulp_points():
    """quad name -> points one ulp inside and one ulp outside of one of its edges (axis-parallel, diagonal, sloped, at the reflex vertex), chosen
    so that every difference and product of the fp64 evaluation is exact"""
    up, dn = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, -math.inf))
    both = lambda f: [f(up), f(dn)]
    return {
        "square": both(lambda f: (2.0, f(0.0))) + both(lambda f: (2.0, f(4.0))) + both(lambda f: (f(0.0), 2.0)) + both(lambda f: (f(4.0), 2.0)),
        "square_cw": both(lambda f: (2.0, f(0.0))) + both(lambda f: (f(4.0), 2.0)),
        "sheared": both(lambda f: (1.0, f(1.0))) + both(lambda f: (3.0, f(3.0))) + both(lambda f: (2.0, f(6.0))),
        "diamond": both(lambda f: (3.0, f(1.0))) + both(lambda f: (1.0, f(1.0))) + both(lambda f: (1.0, f(3.0))),
        "arrow": both(lambda f: (2.0, f(1.0))) + both(lambda f: (f(2.0), 2.0)),
        "square_far": both(lambda f: (65538.0, f(65536.0))) + both(lambda f: (f(65540.0), 65538.0)),
        "diamond_far": both(lambda f: (65539.0, f(65537.0))),
    }


# ---- structured sets for the decision kernels
def lattice_set(nx, ny, off=0, period=32, patterns=None):
    """clusters of integer axis-parallel boxes (sides <= EXACT_SIDE) on a lattice of `period`: IoUs 1, 1/2, 1/4, 1/3, nesting, shared edges and
    corners, duplicates with tied confidences.  Every IoU is evaluated exactly by fp64 (iou_bound = 0 wherever the IoU is dyadic): `>=` at
    thresholds 0.5 and 0.25 is tested on exact ties."""
    pats = patterns or [
        [(0, 0, 3, 2), (1, 0, 4, 2)],                      # IoU 1/2 (tie at 0.5)
        [(0, 0, 5, 1), (3, 0, 8, 1)],                      # IoU 1/4 (tie at 0.25)
        [(0, 0, 4, 4), (0, 0, 4, 2), (0, 0, 2, 2)],        # nested chain: 1/2, 1/4, 1/2
        [(0, 0, 4, 4), (0, 0, 4, 4), (0, 0, 4, 4)],        # exact duplicates
        [(0, 0, 4, 4), (4, 0, 8, 4), (4, 4, 8, 8)],        # shared edge, shared corner: IoU 0
        [(0, 0, 4, 4), (2, 0, 6, 4), (4, 0, 8, 4)],        # chain 1/3, 0 (contact)
        [(0, 0, 8, 8), (1, 1, 7, 7), (2, 2, 6, 6), (3, 3, 5, 5)],  # nesting 36/64, 16/36 ...
        [(0, 0, 16, 16), (0, 0, 16, 8), (8, 0, 16, 8), (0, 8, 16, 16)],  # touches the period's cell borders
    ]
    boxes, cls, conf = [], [], []
    k = 0
    for j in range(ny):
        for i in range(nx):
            for m, (x0, y0, x1, y1) in enumerate(pats[(i + 3 * j) % len(pats)]):
                boxes.append(relabel(box(off + i * period + x0, off + j * period + y0, off + i * period + x1, off + j * period + y1), k % 4, k % 3 == 0))
                cls.append((i + j) % 2)
                conf.append((0.9, 0.8, 0.8, 0.5)[(m + i) % 4] if (i + j) % 3 else 0.75)  # ties inside a cluster: input order decides
                k += 1
    return boxes, cls, conf


def pile_set(seed, n, off=0.0, spread=6.0, ncls=2):
    """`n` random rotated rectangles thrown onto a few heaps: most pairs of a heap overlap heavily"""
    import numpy as np
    rng = np.random.default_rng(seed)
    heaps = max(1, n // 40)
    boxes = []
    for k in range(n):
        hx, hy = (k % heaps) % 8 * 120.0, (k % heaps) // 8 * 120.0
        boxes.append(rect(off + hx + rng.normal(0, spread), off + hy + rng.normal(0, spread), rng.uniform(15, 50), rng.uniform(15, 50), rng.uniform(0, math.pi)))
    return boxes, rng.integers(0, ncls, n).tolist(), np.round(rng.uniform(0.25, 1.0, n), 2).tolist()  # two decimals: confidence ties


# ---- the upper-bound shortcut of merge_segment
def _shoelace_area(q):
    s = 0.0
    for i in range(4):
        j = (i + 1) % 4
        s += q[2 * i] * q[2 * j + 1] - q[2 * j] * q[2 * i + 1]
    return abs(s) * 0.5


def shortcut_skips(a, b, thr, margin="bound"):
    """merge_segment's `ub` test (csrc/geom.hip) restated on the oracle's areas: does the pair never reach the clip?  margin "1e-9": the constant the kernel
    used to have; "bound": the slack in M and E it has now."""
    ai, aj = _shoelace_area(a), _shoelace_area(b)
    ub = min(min(ai, aj), (min(max(a[0::2]), max(b[0::2])) - max(min(a[0::2]), min(b[0::2]))) * (min(max(a[1::2]), max(b[1::2])) - max(min(a[1::2]), min(b[1::2]))))
    if margin == "1e-9":
        return ai + aj - ub > 0.0 and ub * (1.0 + 1e-9) < thr * (ai + aj - ub)
    M = max(abs(c) for c in list(a) + list(b))
    E = sum(max(q[k::2]) - min(q[k::2]) for q in (a, b) for k in (0, 1))
    slack = 2.0 ** -53 * (28.0 * M * M + 256.0 * M * E + 672.0 * E * E)
    return ai + aj - ub - slack > 0.0 and (ub + slack) * (1.0 + 2.0 ** -48) < thr * (ai + aj - ub - slack)


def shortcut_search(margin, oracle_iou):
    """nested thin boxes as the pipeline makes them (float32 local corners + an integer tile offset near 6e4) whose real-number area ratio is
    the threshold; -> the pairs the shortcut skips although the oracle's IoU is >= thr"""
    import numpy as np
    rng = np.random.default_rng(7)
    found = []
    for n in range(3000):
        thr = (0.5, 0.25)[n & 1]
        ox, oy = int(rng.integers(60000, 65536)), int(rng.integers(60000, 65536))
        w, h = float(np.float32(rng.uniform(0.5, 3.0))), float(np.float32(rng.uniform(20, 80)))
        x0, y0, k = ox + float(np.float32(rng.uniform(0, 300))), oy + float(np.float32(rng.uniform(0, 300))), 1.0 / thr
        dx = float(np.float32(rng.uniform(0, w * (k - 1))))
        big, small = box(x0, y0, x0 + w * k, y0 + h), box(x0 + dx, y0, x0 + dx + w, y0 + h)
        for a, b in ((big, small), (small, big)):
            if oracle_iou(a, b) >= thr and shortcut_skips(a, b, thr, margin):
                found.append((a, b, thr))
    return found
