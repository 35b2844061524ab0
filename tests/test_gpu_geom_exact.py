"""The geometry kernels (csrc/geom.hip, geom_device.h) against the exact rational reference of geom_exact.py: polygon IoU on every family of
test_geom_exact_cpu.py, point-in-quad on the validity table, and every kernel that decides from an IoU on structured sets whose every pair the
reference alone can decide (undecided == 0).  Outputs sit between guard bands (bounds.Guarded)."""
import numpy as np
import pytest
import torch

import geom_exact as gx
from bounds import Guarded
from oracle import geom as og
from test_geom_exact_cpu import CONS_CASES, MERGE_CASES, _cons_case, _merge_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops as o
    return o


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


# ------------------------------------------------------------------------------------------------ guarded calls
def g_pairs(ops, a, b):
    out = Guarded((len(a),), torch.float64)
    ops._O.poly_iou_pairs(dev(a, torch.float64), dev(b, torch.float64), out.out)
    return out.get("poly_iou_pairs").cpu().numpy()


def g_matrix(ops, a, b, ca=None, cb=None):
    out = Guarded((len(a), len(b)), torch.float64)
    ops._O.poly_iou_matrix(dev(a, torch.float64), None if ca is None else dev(ca, torch.int32), dev(b, torch.float64),
                           None if cb is None else dev(cb, torch.int32), out.out)
    return out.get("poly_iou_matrix").cpu().numpy()


def g_merge(ops, boxes, cls, conf, thr):
    n = len(boxes)
    order, keep, nk = Guarded((n,), torch.int32), Guarded((n,), torch.uint8), Guarded((1,), torch.int32)
    ops._O.merge_detections(dev(boxes, torch.float64), dev(cls, torch.int32), dev(conf, torch.float64), float(thr), order.out, keep.out, nk.out)
    return order.get("merge order").cpu().tolist(), keep.get("merge keep").cpu().tolist(), int(nk.get("merge n_keep")[0])


def g_segments(ops, boxes, cls, conf, off, thr):
    n = len(boxes)
    order, keep = Guarded((n,), torch.int32), Guarded((n,), torch.uint8, init=torch.zeros(n, dtype=torch.uint8))
    ops._O.merge_segments(dev(boxes, torch.float64), dev(cls, torch.int32), dev(conf, torch.float64), dev(off, torch.int32), float(thr), order.out, keep.out)
    return order.get("segments order").cpu().tolist(), keep.get("segments keep").cpu().tolist()


def g_consensus(ops, boxes, cls, conf, off, thr):
    n = len(boxes)
    out, nout = Guarded((n,), torch.int32, init=torch.full((n,), -1, dtype=torch.int32)), Guarded((1,), torch.int32, init=torch.zeros(1, dtype=torch.int32))
    ops._O.consensus(dev(boxes, torch.float64), dev(cls, torch.int32), dev(conf, torch.float64), [int(o) for o in off], float(thr), 0.25, 0.70, out.out, nout.out)
    k = int(nout.get("consensus n_out")[0])
    return out.get("consensus out")[:k].cpu().tolist()


# ------------------------------------------------------------------------------------------------ IoU
@pytest.mark.parametrize("name", gx.FAMILIES)
def test_iou_pairs_and_matrix_against_exact(ops, name):
    """tolerance 0 on families (a), (b), iou_bound elsewhere; bit-equal to the oracle; batches of 1, 63, 64, 65, 257 and the whole family"""
    fam = gx.family(name)
    A, B = np.array(fam["A"]), np.array(fam["B"])
    ref = og.poly_iou_pairs(A, B)
    got = g_pairs(ops, A, B)
    gx.check_family(name, got, "device pairs")
    assert np.array_equal(got, ref)
    for m in (1, 63, 64, 65, 257):
        assert np.array_equal(g_pairs(ops, A[7:7 + m], B[7:7 + m]), ref[7:7 + m]), m
    # matrix: its diagonal is the family's pairs, the whole of it the oracle's; 65 x 63 = more than one 16 x 16 block per axis, ragged edges
    na, nb = 65, 63
    full = np.array([[og.compute_polygon_iou(a, b) for b in B[:nb]] for a in A[:na]])
    got = g_matrix(ops, A[:na], B[:nb])
    assert np.array_equal(got, full)
    diag = np.array(list(np.diagonal(got)) + list(ref[nb:]))
    gx.check_family(name, diag, "device matrix diagonal")
    ca, cb = (np.arange(na) % 3).astype(np.int32), (np.arange(nb) % 2).astype(np.int32)
    assert np.array_equal(g_matrix(ops, A[:na], B[:nb], ca, cb), np.where(ca[:, None] == cb[None, :], full, 0.0))
    assert np.array_equal(g_matrix(ops, A[:1], B[:1]), full[:1, :1])


def test_points_in_quads_table(ops):
    names = list(gx.TABLE_QUADS)
    quads = np.array([gx.TABLE_QUADS[k] for k in names], np.float64)
    pts = gx.table_points()
    out = Guarded((len(pts), len(names)), torch.uint8)
    ops._O.points_in_quads(dev(np.array(pts), torch.float64), None, dev(quads, torch.float64), None, out.out)
    got = out.get("points_in_quads").cpu().numpy()
    exp = np.array([[gx.point_strictly_inside(q, x, y) for q in quads] for (x, y) in pts], np.uint8)
    assert np.array_equal(got, exp) and exp.sum() > 200
    for name, pp in gx.table_ulp_points().items():  # one ulp inside / outside of an edge
        q = gx.TABLE_QUADS[name]
        out = Guarded((len(pp), 1), torch.uint8)
        ops._O.points_in_quads(dev(np.array(pp), torch.float64), None, dev(np.array([q], np.float64), torch.float64), None, out.out)
        assert out.get(name).cpu().flatten().tolist() == [gx.point_strictly_inside(q, x, y) for (x, y) in pp], name
    # validity as the IoU kernels see it: non-zero iff valid; and the value, against a hull box in both operand orders: the nearest double of
    # the exact IoU (integer operands: the triangles with a repeated vertex and the collinear vertex among them) and the oracle's bits
    self_iou = g_pairs(ops, quads, quads)
    assert [(v != 0.0) for v in self_iou] == [gx.valid(q) for q in quads]
    hulls = np.array([gx.table_hull(k) for k in names], np.float64)
    exact = np.array([gx.iou(q, h)[1] for q, h in zip(quads, hulls)])
    assert (exact != 0.0).tolist() == [gx.valid(q) for q in quads]
    for a, b in ((quads, hulls), (hulls, quads)):
        got = g_pairs(ops, a, b)
        assert np.array_equal(got, exact) and np.array_equal(got, og.poly_iou_pairs(a, b))
    assert np.array_equal(np.diagonal(g_matrix(ops, quads, hulls)), exact)


# ------------------------------------------------------------------------------------------------ decisions
def _exact_merge(boxes, cls, conf, thr):
    (order, keep), undecided = gx.greedy_merge(boxes, cls, conf, thr)
    assert undecided == 0, "the reference alone must decide every pair of this set"
    return order, keep


@pytest.mark.parametrize("case", MERGE_CASES)
def test_merge_below_the_grid_threshold(ops, case):
    """n <= 256 and <= 512: the two LDS-resident forms; the same sets through nms_mask + nms_reduce"""
    boxes, cls, conf, thr = _merge_case(case)
    order, keep = _exact_merge(boxes, cls, conf, thr)
    assert len(boxes) <= 256
    go, gk, nk = g_merge(ops, boxes, cls, conf, thr)
    assert go == order and gk == keep and nk == sum(keep)
    sb, sc = np.array(boxes)[order], np.array(cls, np.int32)[order]
    n = len(boxes)
    mask = Guarded(((n + 63) // 64, n), torch.int64, init=torch.zeros(((n + 63) // 64, n), dtype=torch.int64))
    ops._O.nms_mask(dev(sb, torch.float64), dev(sc, torch.int32), float(thr), mask.out)
    k2 = Guarded((n,), torch.uint8)
    nk2 = Guarded((1,), torch.int32)
    ops._O.nms_reduce(mask.get("nms_mask"), n, k2.out, nk2.out)
    assert k2.get("nms_reduce keep").cpu().tolist() == keep and int(nk2.get("nms_reduce n")[0]) == sum(keep)


def _big_lattice(nx, ny, extra_large):
    boxes, cls, conf = gx.lattice_set(nx, ny, off=1024)
    for k in range(extra_large):  # boxes larger than a grid cell (sides <= EXACT_SIDE keep the IoUs exact: larger ones are far from everything but each other)
        x, y = 1024 + 320 * k, 1024 + 32 * ny + 64
        boxes += [gx.box(x, y, x + 300, y + 200), gx.box(x + 10, y + 10, x + 290, y + 190)]
        cls += [0, 0]
        conf += [0.95, 0.6]
    return boxes, cls, conf


@pytest.mark.parametrize("case,thr", [("mid_400", 0.5), ("dense_700", 0.25), ("grid_8412", 0.5), ("overflow", 0.5)])
def test_merge_dense_grid_and_overflow(ops, case, thr):
    """400 rows: the 512-row LDS form; 700: k_nms_mask's pair list; > 8192: k_grid_pairs (period-32 lattice: boxes on cell borders, plus boxes
    larger than a cell); overflow: more suppressing pairs than the pair list holds (k_nms_lazy)"""
    if case == "mid_400":
        boxes, cls, conf = gx.lattice_set(14, 11)
        boxes, cls, conf = boxes[:400], cls[:400], conf[:400]
    elif case == "dense_700":
        boxes, cls, conf = gx.lattice_set(17, 14)
        boxes, cls, conf = boxes[:700], cls[:700], conf[:700]
    elif case == "grid_8412":
        boxes, cls, conf = _big_lattice(56, 50, 6)
        assert len(boxes) == 8412
    else:
        boxes, cls, conf = gx.lattice_set(4, 4)
        boxes, cls, conf = boxes + [gx.box(500, 500, 504, 504)] * 700, cls + [0] * 700, conf + [0.5] * 700  # 244 650 pairs > 64 n + 4096
    order, keep = _exact_merge(boxes, cls, conf, thr)
    go, gk, nk = g_merge(ops, boxes, cls, conf, thr)
    assert go == order and gk == keep and nk == sum(keep)
    assert 0 < sum(keep) < len(keep)


def test_merge_segments_lengths_and_candidate_overflow(ops):
    """segments of 1, 64, 65, 512 and 513 rows, one whose candidate list overflows kSegPairCap (200 overlapping same-class boxes: 19 900
    candidate pairs), one at offset 65 536; each against the exact greedy merge of its own rows"""
    segs = []
    for n, off in ((1, 0), (64, 0), (65, 65536), (512, 0), (513, 65536)):
        b, c, s = gx.lattice_set(16, 12, off=off)
        assert len(b) >= n
        segs.append((b[:n], c[:n], s[:n]))
    crowd = [gx.box(0, 0, 8, 8), gx.box(0, 0, 8, 4), gx.box(0, 0, 4, 4), gx.box(1, 0, 9, 8)]
    segs.append(([crowd[k % 4] for k in range(200)], [0] * 200, [0.5 + (k % 7) / 16 for k in range(200)]))
    b, c, s = gx.pile_set(21, 130, off=65536.0)
    segs.append((b, c, s))
    for thr in (0.5, 0.25):
        boxes, cls, conf, off, order, keep = [], [], [], [0], [], []
        for (b, c, s) in segs:
            o, k = _exact_merge(b, c, s, thr)
            order += [off[-1] + i for i in o]
            keep += k
            boxes, cls, conf = boxes + b, cls + c, conf + s
            off.append(len(boxes))
        go, gk = g_segments(ops, boxes, cls, conf, off, thr)
        assert go == order and gk == keep


@pytest.mark.parametrize("case", CONS_CASES + ("parallel_lattice", "parallel_piles"))
def test_consensus_walk_and_parallel_form(ops, case):
    """<= 512 rows: the walk; above: the parallel form.  Both with confidence ties (lattice_set, pile_set)."""
    if case == "parallel_lattice":
        b, c, s = gx.lattice_set(12, 10)
        b2, c2, s2 = gx.lattice_set(12, 10, patterns=[[(0, 0, 4, 4), (1, 0, 4, 4)], [(0, 0, 5, 2), (0, 0, 2, 2)], [(0, 0, 4, 4)], [(2, 0, 6, 4), (2, 0, 6, 4)]])
        boxes, cls, conf, off, thr = b + b2, c + c2, s + s2, [0, len(b), len(b) + len(b2)], 0.5
    elif case == "parallel_piles":
        boxes, cls, conf = gx.pile_set(9, 540, spread=14.0)
        off, thr = [0, 220, 400, 540], 0.4
    else:
        boxes, cls, conf, off, thr = _cons_case(case)
    assert (len(boxes) > 512) == case.startswith("parallel")
    out, undecided = gx.consensus(boxes, cls, conf, off, iou_partner=thr)
    assert undecided == 0, "the reference alone must decide every pair of this set"
    assert g_consensus(ops, boxes, cls, conf, off, thr) == out
    assert 0 < len(out) < len(boxes)


def test_upper_bound_shortcut_pairs_through_merge_segments(ops):
    """the pairs test_geom_exact_cpu.py found: their exact IoU ties the threshold (undecided for the exact reference), the oracle's fp64 value is
    >= thr, and the constant-margin shortcut skipped them.  merge_segments and merge_detections must decide as the oracle does."""
    found = gx.shortcut_search("1e-9", og.compute_polygon_iou)[:6]
    assert len(found) == 6
    filler, _, _ = gx.lattice_set(6, 4)  # 70 far rows of another class: the segment is longer than a wave takes (the wave kernel has no shortcut)
    filler = filler[:70]
    for (a, b, thr) in found:
        boxes, cls, conf = [a, b] + filler, [7, 7] + [1] * 70, [0.9, 0.8] + [0.5] * 70
        o, k = og.merge_arrays(np.array(boxes), np.array(cls, np.int32), np.array(conf), thr)
        assert k[1] == 0  # the oracle suppresses b
        go, gk = g_segments(ops, boxes, cls, conf, [0, len(boxes)], thr)
        assert go == list(o) and gk == list(k)
        go, gk, _ = g_merge(ops, boxes, cls, conf, thr)
        assert go == list(o) and gk == list(k)
