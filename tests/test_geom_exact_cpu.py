"""The CPU oracle's geometry (oracle/obb_oracle.c: polygon IoU, validity, point-in-quad, the greedy merge and the consensus walk) against the
exact rational reference of geom_exact.py -- runs without a GPU.  The device kernels are held to the same reference in test_gpu_geom_exact.py."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import geom_exact as gx
from oracle import geom as og


# ------------------------------------------------------------------------------------------------ the reference checks itself
def test_closed_forms():
    sq = gx.box(0, 0, 1, 1)
    assert gx.iou(sq, gx.box(0.5, 0, 1.5, 1))[0] == F(1, 3)
    assert gx.iou(sq, sq) == (F(1), 1.0)
    assert gx.iou(sq, gx.box(1, 0, 2, 1))[0] == 0 and gx.iou(sq, gx.box(2, 2, 3, 3))[0] == 0  # contact, disjoint
    assert gx.iou(gx.box(0, 0, 10, 10), gx.box(4, 3, 6, 7))[0] == F(8, 100)  # containment: the area ratio
    assert gx.iou(gx.box(0, 0, 4, 4), [2, 0, 4, 2, 2, 4, 0, 2])[0] == F(1, 2)  # the inscribed diamond
    assert gx.iou(gx.box(0, 0, 4, 4), [2, -2, 6, 2, 2, 6, -2, 2])[0] == F(16, 32)  # the circumscribed one
    assert gx.iou(gx.box(1, 1, 5, 5), [2, 0, 4, 2, 2, 4, 0, 2])[0] == F(6, 16 + 8 - 6)  # the diamond (area 8) loses two corner triangles of area 1
    arrow, sq2 = [0, 0, 2, 1, 0, 2, 1, 1], gx.box(0, 0, 2, 2)  # the arrow-head of test_oracle_geometry.py: area 1
    assert gx.iou(arrow, sq2)[0] == F(1, 4) and gx.iou(arrow, arrow)[0] == 1
    # arrow x (arrow + 1/2) by hand: arrow = T minus N, T the outer triangle (0,0)(2,1)(0,2), N the notch triangle (0,0)(1,1)(0,2); primes = shifted.
    # |T n T'| = 25/32 (T' = T scaled by 3/4 about its tip, cut by x >= 1/2 ... the triangle (1/2,1/2)(2,1)... similar to T with ratio 5/8 ... area 2 (5/8)^2),
    # |T n N'| = 25/48, |N n T'| = 1/4 (the triangle (1/2,1/2)(1,1)(1/2,3/2)), |N n N'| = 1/4 (the same triangle):
    # intersection = 25/32 - 25/48 - 1/4 + 1/4 = 25/96, union = 2 - 25/96 = 167/96, IoU = 25/167.
    assert gx.iou(arrow, [v + 0.5 for v in arrow])[0] == F(25, 167)


def test_fp64_multiplication_undoes_division_up_to_the_exact_side():
    """the lemma iou_bound's exact case rests on: fl(n fl(k / n)) == k for 0 <= k <= n <= EXACT_SIDE (it first fails at 22 * (15 / 22))"""
    assert all(n * (k / n) == k for n in range(1, gx.EXACT_SIDE + 1) for k in range(n + 1))
    assert 22 * (15 / 22) != 15


def test_symmetry_and_relabelling_are_exact():
    for name in ("c", "e"):
        fam = gx.family(name)
        for k in range(0, len(fam["A"]), 15):
            a, b, ex = fam["A"][k], fam["B"][k], fam["exact"][k]
            assert gx.iou(b, a)[0] == ex
            assert gx.iou(gx.relabel(a, 1 + k % 3, False), gx.relabel(b, k % 4, True))[0] == ex
            assert gx.iou(gx.relabel(a, k % 4, True), b)[0] == ex


# ------------------------------------------------------------------------------------------------ the oracle against the exact value
@pytest.mark.parametrize("name", gx.FAMILIES)
def test_oracle_iou_against_exact(name):
    """|oracle - exact| is 0 in double on families (a), (b) and within iou_bound elsewhere; every family reaches its intended paths.
    Measured worst |err| / iou_bound: (c) 0.26, (d) 0.17, (e) 0.012, (f) 0.23, (g) 0.09 -- see DESIGN.md, "polygon IoU"."""
    fam = gx.family(name)
    gx.check_family(name, og.poly_iou_pairs(np.array(fam["A"]), np.array(fam["B"])), "oracle")
    gx.check_family(name, og.poly_iou_pairs(np.array(fam["B"]), np.array(fam["A"])), "oracle, operands swapped")
    if name not in gx.ZERO_TOLERANCE:  # a bound this small catches a swapped vertex or a dropped clip stage (>= 1e-3 on these inputs)
        assert sorted(fam["bound"])[len(fam["bound"]) // 2] < 1e-6


# ---- a Python twin of the oracle's clip, to show that the bounds catch what they must
def _twin_iou(b1, b2, skip_edge=False, strict=False, wrong_fan=False):
    cross = lambda a, b, c: (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])

    def shoe(p):
        s = 0.0
        for i in range(len(p)):
            j = 0 if i + 1 == len(p) else i + 1
            s += p[i][0] * p[j][1] - p[j][0] * p[i][1]
        return s

    def convex(p):
        c = [cross(p[i], p[(i + 1) % 4], p[(i + 2) % 4]) for i in range(4)]
        return not (any(v > 0 for v in c) and any(v < 0 for v in c))

    def clip(subj, cl):
        cur = list(subj)
        for e in range(len(cl) - (1 if skip_edge else 0)):
            a, b = cl[e], cl[(e + 1) % len(cl)]
            if not cur:
                break
            out, s = [], cur[-1]
            ds = cross(a, b, s)
            for p in cur:
                dp = cross(a, b, p)
                cut = lambda: (s[0] + (p[0] - s[0]) * (ds / (ds - dp)), s[1] + (p[1] - s[1]) * (ds / (ds - dp)))
                if (dp > 0.0) if strict else (dp >= 0.0):
                    if ds < 0.0:
                        out.append(cut())
                    out.append(p)
                elif ds >= 0.0 and ds != dp:
                    out.append(cut())
                s, ds = p, dp
            cur = out
        return abs(shoe(cur)) * 0.5 if len(cur) >= 3 else 0.0

    def tris(q):
        r = -1
        for i in range(4):
            if cross(q[i - 1], q[i], q[(i + 1) % 4]) < 0.0:
                r = i
        s = 0 if r < 0 else ((r + 1) % 4 if wrong_fan else r)
        return [[q[s], q[(s + 1) % 4], q[(s + 2) % 4]], [q[s], q[(s + 2) % 4], q[(s + 3) % 4]]]

    p, q = [(b1[2 * i], b1[2 * i + 1]) for i in range(4)], [(b2[2 * i], b2[2 * i + 1]) for i in range(4)]
    a1, a2 = abs(shoe(p)) * 0.5, abs(shoe(q)) * 0.5
    p, q = (p[::-1] if shoe(p) < 0.0 else p), (q[::-1] if shoe(q) < 0.0 else q)
    if convex(q):
        inter = clip(p, q)
    elif convex(p):
        inter = clip(q, p)
    else:
        inter = sum(clip(s, t) for s in tris(p) for t in tris(q))
    uni = a1 + a2 - inter
    return inter / uni if uni > 0.0 else 0.0


def _families_failed(**mutation):
    failed = []
    for name in gx.FAMILIES:
        fam = gx.family(name)
        try:
            gx.check_family(name, [_twin_iou(a, b, **mutation) for a, b in zip(fam["A"], fam["B"])], f"twin {mutation}")
        except AssertionError:
            failed.append(name)
    return failed


def test_the_bounds_catch_three_mutations_of_the_clip():
    assert _families_failed() == []  # the unmutated twin passes everywhere
    assert _families_failed(skip_edge=True), "a skipped clip edge went unnoticed"
    assert _families_failed(strict=True), "'>=' turned into '>' on the inside test went unnoticed"
    assert "e" in _families_failed(wrong_fan=True), "a wrong fan vertex in the concave split went unnoticed"


# ------------------------------------------------------------------------------------------------ validity and point-in-quad
def test_validity_and_point_in_quad_table():
    expect_valid = {"square", "square_cw", "diamond", "sheared", "arrow", "collinear_vertex", "repeated_first", "repeated_mid", "repeated_wrap",
                    "square_far", "diamond_far"}
    pts, ulp = gx.table_points(), gx.table_ulp_points()
    for name, pp in ulp.items():  # each pair of points straddles an edge: one inside, one outside, and the oracle agrees on every one
        assert [gx.point_strictly_inside(gx.TABLE_QUADS[name], x, y) for (x, y) in pp].count(1) == len(pp) // 2, name
        for (x, y) in pp:
            assert int(og.point_in_quad(gx.TABLE_QUADS[name], x, y)) == gx.point_strictly_inside(gx.TABLE_QUADS[name], x, y), (name, x, y)
    hits = 0
    for name, q in gx.TABLE_QUADS.items():
        assert gx.valid(q) == (name in expect_valid), name
        # the zero / non-zero pattern of the IoU is the validity
        hull = gx.table_hull(name)
        assert (og.compute_polygon_iou(q, q) != 0.0) == gx.valid(q), name
        assert (og.compute_polygon_iou(q, hull) != 0.0) == gx.valid(q) and (og.compute_polygon_iou(hull, q) != 0.0) == gx.valid(q), name
        if gx.valid(q):
            assert og.compute_polygon_iou(q, hull) == gx.iou(q, hull)[1] and og.compute_polygon_iou(hull, q) == gx.iou(hull, q)[1], name
        for (x, y) in pts:
            ex = gx.point_strictly_inside(q, x, y)
            assert int(og.point_in_quad(q, x, y)) == ex, (name, x, y)
            hits += ex
    assert hits > 200
    # one ulp decides: just inside and just outside of the square's lower edge, exactly on it
    sq = gx.TABLE_QUADS["square"]
    ys = (math.nextafter(0.0, 1.0), 0.0, math.nextafter(0.0, -1.0))
    assert [gx.point_strictly_inside(sq, 2.0, y) for y in ys] == [1, 0, 0] and [int(og.point_in_quad(sq, 2.0, y)) for y in ys] == [1, 0, 0]


# ------------------------------------------------------------------------------------------------ decisions
def _merge_case(name):
    if name == "lattice_0.5":
        return gx.lattice_set(6, 5) + (0.5,)
    if name == "lattice_0.25":
        return gx.lattice_set(6, 5) + (0.25,)
    if name == "lattice_far_0.5":
        return gx.lattice_set(5, 4, off=65536) + (0.5,)
    if name == "pile":
        return gx.pile_set(3, 90) + (0.4,)
    if name == "pile_far":
        return gx.pile_set(4, 80, off=65536.0) + (0.4,)
    if name == "thr0":
        return gx.lattice_set(4, 4) + (0.0,)
    raise KeyError(name)


MERGE_CASES = ("lattice_0.5", "lattice_0.25", "lattice_far_0.5", "pile", "pile_far", "thr0")


@pytest.mark.parametrize("case", MERGE_CASES)
def test_oracle_merge_against_exact_greedy(case):
    boxes, cls, conf, thr = _merge_case(case)
    (order, keep), undecided = gx.greedy_merge(boxes, cls, conf, thr)
    assert undecided == 0, "the reference alone must decide every pair of this set"
    o, k = og.merge_arrays(np.array(boxes), np.array(cls, np.int32), np.array(conf), thr)
    assert list(o) == order and list(k) == keep
    assert 0 < sum(keep) < len(keep)


def _cons_case(name):
    if name == "lattice":
        b, c, s = gx.lattice_set(6, 5)
        b2, c2, s2 = gx.lattice_set(6, 5, patterns=[[(0, 0, 4, 4), (1, 0, 4, 4)], [(0, 0, 5, 2), (0, 0, 2, 2)], [(0, 0, 4, 4)], [(2, 0, 6, 4), (2, 0, 6, 4)]])
        return b + b2, c + c2, s + s2, [0, len(b), len(b) + len(b2)], 0.4
    if name == "lattice_tie_0.5":
        b, c, s = gx.lattice_set(5, 4, off=65536)
        b2, c2, s2 = gx.lattice_set(5, 4, off=65536, patterns=[[(0, 0, 4, 2)], [(0, 0, 4, 4), (0, 0, 2, 4)], [(4, 0, 8, 4)]])
        return b + b2, c + c2, s + s2, [0, len(b), len(b) + len(b2)], 0.5
    if name == "piles":
        b, c, s = gx.pile_set(8, 120, spread=9.0)
        return b, c, s, [0, 50, 90, 120], 0.4
    raise KeyError(name)


CONS_CASES = ("lattice", "lattice_tie_0.5", "piles")


@pytest.mark.parametrize("case", CONS_CASES)
def test_oracle_consensus_against_exact_walk(case):
    boxes, cls, conf, off, thr = _cons_case(case)
    out, undecided = gx.consensus(boxes, cls, conf, off, iou_partner=thr)
    assert undecided == 0, "the reference alone must decide every pair of this set"
    got = og.consensus_arrays(np.array(boxes), np.array(cls, np.int32), np.array(conf), off, iou_partner=thr)
    assert list(got) == out
    assert 0 < len(out) < len(boxes)


# ------------------------------------------------------------------------------------------------ the upper-bound shortcut of merge_segment
def test_upper_bound_shortcut_never_skips_a_hit():
    """Outcome of the search (seed 7, 3000 nested pairs, both operand orders, M ~ 6e4): with the constant margin `ub (1 + 1e-9) < thr den`
    the shortcut skipped 1298 pairs whose oracle IoU is >= thr (for instance IoU 0.25000000030 at thr 0.25: the areas carry ~1e-8 relative
    at these coordinates, not 1e-15) -- merge_segments then kept a box the oracle suppresses.  With the margin derived from M and the
    extents it skips none.  The first six finds are a GPU case (test_gpu_geom_exact.py)."""
    old = gx.shortcut_search("1e-9", og.compute_polygon_iou)
    print(f"  constant margin: {len(old)} wrongly skipped pairs; derived margin: ", end="")
    assert len(old) > 0, "the search no longer reproduces what motivated the derived margin"
    new = gx.shortcut_search("bound", og.compute_polygon_iou)
    print(len(new))
    assert new == []
    # the derived margin still skips what it is there for: pairs far below the threshold
    fam = gx.family("c")
    far_below = [(a, b) for a, b, e in zip(fam["A"], fam["B"], fam["nearest"]) if 0.0 < e < 0.2]
    assert sum(gx.shortcut_skips(a, b, 0.4) for a, b in far_below) > 0
    # ... and the exact reference says why the oracle is the yardstick for these pairs: their exact IoU is a tie the fp64 evaluation cannot decide
    a, b, thr = old[0]
    ex = gx.iou(a, b)
    assert gx.cannot_decide(ex[0], thr, gx.iou_bound(a, b, ex))
