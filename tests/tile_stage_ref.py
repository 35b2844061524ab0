"""Reference and case builders for the per-tile survivor stage (csrc/post_device.h `tile_post_row`; csrc/geom.hip `k_tile_stage`,
`k_scan_counts`, `k_tile_emit`, `k_records_to_dets`, `k_kept_*`, `k_gather_compact`).  Host only: Python floats (IEEE double), numpy
and the exact rational merge of geom_exact.py.  Shared by test_tile_stage_cpu.py and test_gpu_tile_stage.py.

  post_row(lp, cls, rect, margin, strike_cls)   tile_post_row restated: one IEEE operation per step, in the kernel's order
  stage(local_pts, cls, conf32, count, ...)     expected records / tile_off / n_records of obb_tile_survivors + the undecided pair count
  dets_of(records, n, rects, strike_cls)        expected output of obb_records_to_dets
  check_stage / check_post                      the comparisons of the GPU test (the CPU test runs its stand-in through the same ones)
  case(name), CASES, angle_table()              the committed cases

Where the local corners come from: `stage` takes the fp32 corners as an argument.  The GPU test passes the bits of the device's own
`ops.results` on the same rows (cosf / sinf bits cannot be restated here; that kernel is held per element by
test_results_every_element_within_the_derived_bound); the CPU test passes `results_host`, which equals those bits wherever a case is
marked `exact`: angle 0 or (float)(pi / 2) (regularised to 0 with the sides swapped), no letterbox, integer centres and even sides, so
that cos = 1 and sin = 0 exactly and every corner is an integer.  From the corner bits on, everything here is exact."""
import functools
import math

import numpy as np

import geom_exact as gx

K_DEG = 180.0 / 3.141592653589793
PI_F = np.float32(3.14159274101257324)
HALF_PI_F = np.float32(1.57079637050628662)
FILL = -1  # an int32 of a guard-filled (0xff) buffer
ANGLE_TOL = 1e-9  # degrees: the band test_gpu_geometry.py allows the device's atan2
ANGLE_SEP = 1e-3  # degrees: every angle case is at least this far from what a wrong rule gives
GARBAGE = (np.nan, np.nan, np.nan, np.nan, 2.0, 1e6, np.nan)  # rows past the count: must reach nothing

# tile table shared by the cases (x, y, x2, y2).  A slot's tile id indexes this table and is never the slot index by construction.
RECTS = np.array([[0, 0, 416, 416], [31584, 316, 32000, 732], [316, 31584, 444, 31712], [0, 632, 416, 642], [316, 0, 732, 416],
                  [632, 316, 1048, 732], [100, 100, 228, 228]], np.int32)
T416_FAR, T128_FAR, T_THIN, T128 = 1, 2, 3, 6


def bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ the reference
def post_row(lp, cls, rect, margin, strike_cls):
    """tile_post_row: -> (global corners [8], angle, inside).  Python floats are IEEE doubles; each line is one operation of the kernel."""
    x, y, x2, y2 = (int(v) for v in rect)
    p = [float(v) for v in lp]  # widen
    g = [p[k] + float(x if k % 2 == 0 else y) for k in range(8)]  # add the integer offset
    cx, cy = (g[0] + g[2] + g[4] + g[6]) / 4.0, (g[1] + g[3] + g[5] + g[7]) / 4.0
    cxr, cyr, m = cx - float(x), cy - float(y), float(margin)
    cw, ch = float(x2 - x), float(y2 - y)
    inside = True
    if margin > 0:
        inside = (m <= cxr and cxr <= cw - m) and (m <= cyr and cyr <= ch - m)
    a = 0.0
    if int(cls) == int(strike_cls):  # from the LOCAL corners
        a = math.atan2(p[6] - p[0], p[7] - p[1]) * K_DEG
        a = 180 - a if a > 0 else abs(a)
    return g, a, inside


_MERGES = {}


def merge(boxes, cls, conf, thr):
    """gx.greedy_merge, remembered per input (the scan cases repeat a few tiles thousands of times) -> ((order, keep), undecided)"""
    if not len(boxes):
        return ([], []), 0
    key = (np.asarray(boxes, np.float64).tobytes(), tuple(int(c) for c in cls), tuple(float(c) for c in conf), float(thr))
    if key not in _MERGES:
        _MERGES[key] = gx.greedy_merge([list(b) for b in boxes], list(cls), list(conf), thr)
    return _MERGES[key]


def stage(local_pts, cls, conf32, count, tile_ids, rects, margin, thr, strike_cls):
    """Expected output of obb_tile_survivors.  local_pts float32 [B, md, 8], cls int [B, md], conf32 float32 [B, md].
    -> dict(records int32 [n, 12] = (tile id, cls, conf bits, 0, 8 corner bits) in order, tile_off int32 [B + 1], n_records, undecided,
    survivors [B], kept [B]).  B = 0 writes n_records only: tile_off is then the guard fill."""
    B, md = np.asarray(cls).shape
    lp32, cf32 = np.ascontiguousarray(local_pts, np.float32), np.ascontiguousarray(conf32, np.float32)
    rows, off, undecided, survivors, kept = [], [0], 0, [], []
    for t in range(B):
        tile = int(tile_ids[t])
        surv, gs = [], []
        for k in range(min(int(count[t]), md)):
            g, _, inside = post_row(lp32[t, k], cls[t][k], rects[tile], margin, strike_cls)
            if inside:
                surv.append(k), gs.append(g)
        (order, keep), u = merge(gs, [int(cls[t][k]) for k in surv], [float(cf32[t, k]) for k in surv], thr)  # widened fp32 confidence, stable descending
        undecided += u
        mine = [surv[o] for o, kf in zip(order, keep) if kf]  # the kept rows in merge order
        for k in mine:
            rows.append([tile, int(cls[t][k]), int(cf32[t, k].view(np.int32)), 0] + bits(lp32[t, k]).tolist())
        off.append(len(rows))
        survivors.append(len(surv)), kept.append(len(mine))
    return {"records": np.array(rows, np.int32).reshape(-1, 12), "tile_off": np.array(off if B else [FILL], np.int32), "n_records": len(rows),
            "undecided": undecided, "survivors": survivors, "kept": kept}


def dets_of(records, n, rects, strike_cls):
    """Expected output of obb_records_to_dets on the first n record rows: -> (gboxes float64 [n, 8], cls int32 [n], conf float64 [n], angle [n])"""
    rec = np.asarray(records, np.int32).reshape(-1, 12)[:n]
    gb, ang = np.zeros((n, 8)), np.zeros(n)
    for i, r in enumerate(rec):
        gb[i], ang[i], _ = post_row(r[4:12].view(np.float32), r[1], rects[r[0]], 0, strike_cls)
    return gb, rec[:, 1].copy(), rec[:, 2].copy().view(np.float32).astype(np.float64), ang


# ------------------------------------------------------------------------------------------------ the comparisons
def check_stage(what, rec, off, n, exp):
    """records[:n], tile_off and n_records equal the reference as int32 bits; off[t + 1] - off[t] is the slot's kept count; rows at and past
    n_records are still the guard fill.  rec: the whole capacity [B * md, 12]."""
    rec, off, n = np.asarray(rec, np.int32).reshape(-1, 12), np.asarray(off, np.int32), int(n)
    assert n == exp["n_records"], f"{what}: n_records {n}, expected {exp['n_records']}"
    assert np.array_equal(off, exp["tile_off"]), f"{what}: tile_off differs, first at slot {_first_diff(off, exp['tile_off'])}"
    if len(exp["kept"]):
        assert np.array_equal(np.diff(off), np.array(exp["kept"], np.int32)), f"{what}: tile_off steps are not the kept counts"
        assert int(off[-1]) == n
    assert 0 <= n <= len(rec), f"{what}: n_records outside the capacity"
    assert np.array_equal(rec[:n], exp["records"]), f"{what}: record row {_first_diff(rec[:n], exp['records'])} differs"
    assert bool((rec[n:] == FILL).all()), f"{what}: a row at or past n_records was written"


def _first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f"(shapes {a.shape} / {b.shape})"
    d = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
    return int(d[0]) if len(d) else None


def check_post(what, g, ang, ins, exp_g, exp_ang, exp_ins=None):
    """global corners (and the inside flag) bit for bit; the angle within ANGLE_TOL degrees"""
    g, exp_g = np.ascontiguousarray(g, np.float64).reshape(-1, 8), np.ascontiguousarray(exp_g, np.float64).reshape(-1, 8)
    assert np.array_equal(g.view(np.int64), exp_g.view(np.int64)), f"{what}: global corners of row {_first_diff(g.view(np.int64), exp_g.view(np.int64))} differ"
    if exp_ins is not None:
        assert np.array_equal(np.asarray(ins).astype(bool), np.asarray(exp_ins).astype(bool)), f"{what}: inside flag differs"
    ang, exp_ang = np.asarray(ang, np.float64), np.asarray(exp_ang, np.float64)
    worst = float(np.abs(ang - exp_ang).max()) if len(ang) else 0.0
    print(f"  {what}: {len(ang)} rows, worst |angle - ref| = {worst:.3e} degrees")
    assert worst <= ANGLE_TOL, f"{what}: angle of row {int(np.abs(ang - exp_ang).argmax())} is {worst:.3e} degrees off"


# ------------------------------------------------------------------------------------------------ result construction on the host
def _py_remainder(a, b):
    r = np.fmod(a, b)
    return np.where((r != 0) & (r < 0), r + b, r).astype(np.float32)


def results_host(det, lb=None):
    """results_row of post_device.h in numpy float32: det [B, md, 7], lb [B, 3] or None -> local corners float32 [B, md, 8].  The device's bits
    wherever cos and sin are exact (the `exact` cases); elsewhere a stand-in that lets the CPU test see the cases (libm cosf is not the
    device's)."""
    d = np.asarray(det, np.float32)
    two = np.float32(2.0)
    with np.errstate(invalid="ignore"):
        x, y, w, h, t = (d[..., k] for k in (0, 1, 2, 3, 6))
        swap = _py_remainder(t, PI_F) >= HALF_PI_F
        w_, h_ = np.where(swap, h, w), np.where(swap, w, h)
        t = _py_remainder(t, HALF_PI_F)
        if lb is not None:
            gain, px, py = (np.asarray(lb, np.float32)[:, k][:, None] for k in range(3))
            x, y, w_, h_ = (x - px) / gain, (y - py) / gain, w_ / gain, h_ / gain
        c, s = np.cos(t), np.sin(t)
        v1x, v1y, v2x, v2y = w_ / two * c, w_ / two * s, -h_ / two * s, h_ / two * c
        p = np.stack([x + v1x + v2x, y + v1y + v2y, x + v1x - v2x, y + v1y - v2y, x - v1x - v2x, y - v1y - v2y, x - v1x + v2x, y - v1y + v2y], -1)
    assert p.dtype == np.float32
    return p


# ------------------------------------------------------------------------------------------------ case builders
def _blank(B, md):
    return np.tile(np.array(GARBAGE, np.float32), (B, md, 1))


def _pos(i, lo=24, pitch=8, per_row=46):
    """the i-th cell of a pitch-8 grid inside the margin of a 416 tile: 4 x 4 boxes on it are 4 px apart (strictly disjoint envelopes)"""
    return lo + pitch * (i % per_row), lo + pitch * (i // per_row)


def _put(det, t, k, cx, cy, w=4, h=4, conf=0.5, cls=0, ang=0.0):
    det[t, k] = (cx, cy, w, h, conf, cls, ang)


def _conf(k):
    return ((k * 37) % 101 + 1) / 128.0  # exact in fp32, not sorted, with ties


def _make(name, det, count, tile_ids, margin, thr=0.5, strike_cls=1, lb=None, exact=True, survivors=None, kept=None, centres=None):
    B = det.shape[0]
    assert len(count) == B and len(tile_ids) == B
    return {"name": name, "det": np.ascontiguousarray(det, np.float32), "count": np.array(count, np.int32), "tile_ids": np.array(tile_ids, np.int32),
            "rects": RECTS, "margin": margin, "thr": thr, "strike_cls": strike_cls, "lb": None if lb is None else np.array(lb, np.float32).reshape(B, 3),
            "exact": exact, "survivors": survivors, "kept": kept, "centres": centres or []}


def _border(name, size, m, tiles):
    """Decided border rows: angle 0 (cos = 1, sin = 0 exactly), sides 4 x 4 (even half sides) and integer centres, so all four corners are
    integers and the centre (a + b + c + d) / 4 is exact.  Centres at m - 1, m, m + 1 and size - m - 1, size - m, size - m + 1 on each
    axis independently (the other coordinate well inside, 10 px apart: no two boxes meet), then the corners of the kept square and rows
    that fail one axis only."""
    edge = (m - 1, m, m + 1, size - m - 1, size - m, size - m + 1)
    ctr = [(v, m + 8 + 10 * j) for j, v in enumerate(edge)] + [(m + 8 + 10 * j, v) for j, v in enumerate(edge)]
    ctr += [(m, m), (size - m, size - m), (m, size - m), (m - 1, size - m - 6), (size - m - 6, size - m + 1), (size - m + 1, m + 6), (m + 6, m - 1)]
    md = len(ctr) + 3
    det = _blank(len(tiles), md)
    centres, surv = [], []
    for t in range(len(tiles)):
        for k, (cx, cy) in enumerate(ctr):
            _put(det, t, k, cx, cy, conf=_conf(k), cls=k % 4)
            centres.append((t, k, cx, cy))
        surv.append(sum(1 for (cx, cy) in ctr if m <= cx <= size - m and m <= cy <= size - m))
    return _make(name, det, [len(ctr)] * len(tiles), tiles, m, survivors=surv, kept=surv, centres=centres)


def _nothing_survives():
    """a 10 x 416 crop with margin 20 (ch - m < m: no centre can pass), a 416 tile whose rows all sit one px outside the margin, an empty slot"""
    det = _blank(3, 40)
    thin = [(208, 5), (20, 5), (396, 5), (208, 0), (208, 10), (100, -10), (100, 20)]
    for k, (cx, cy) in enumerate(thin):
        _put(det, 0, k, cx, cy, cls=k % 3)
    out = [(19, 40 + 10 * k) for k in range(10)] + [(40 + 10 * k, 397) for k in range(10)]
    for k, (cx, cy) in enumerate(out):
        _put(det, 1, k, cx, cy, cls=k % 3)
    cen = [(0, k, cx, cy) for k, (cx, cy) in enumerate(thin)] + [(1, k, cx, cy) for k, (cx, cy) in enumerate(out)]
    return _make("nothing_survives", det, [len(thin), len(out), 0], [T_THIN, T416_FAR, 0], 20, survivors=[0, 0, 0], kept=[0, 0, 0], centres=cen)


def _margin0():
    """margin 0 keeps everything, centres on the edge of and outside the tile included"""
    ctr = [(0, 0), (416, 416), (-50, 500), (1000, -8), (208, 208), (19, 19), (-4, 208)]
    det = _blank(2, 10)
    for t in range(2):
        for k, (cx, cy) in enumerate(ctr):
            _put(det, t, k, cx, cy, conf=_conf(k), cls=k % 3)
    return _make("margin0", det, [len(ctr)] * 2, [T416_FAR, T128_FAR], 0, survivors=[len(ctr)] * 2, kept=[len(ctr)] * 2,
                 centres=[(t, k, cx, cy) for t in range(2) for k, (cx, cy) in enumerate(ctr)])


def _counts(md):
    """count in {-3, 0, md + 7, md, 1} within one batch; the slot after the over-long one holds live rows (an unclamped count would take them)"""
    count = [-3, 0, md + 7, md, 1]
    det = _blank(5, md)
    for t in (2, 3, 4):
        for k in range(min(count[t], md)):
            _put(det, t, k, *_pos(k), conf=_conf(k + t), cls=(k + t) % 4)
    live = [0, 0, md, md, 1]
    return _make(f"counts_md{md}", det, count, [4, 0, T416_FAR, 5, T128_FAR], 20, survivors=live, kept=live)


def _rounds():
    """k_tile_stage compacts in rounds of 256 rows: (0) rows 0..255 fail the border and row 256 passes (carry 0 into round two); 255, 256
    and 257 of 300 rows pass, the failing ones spread over both rounds; 512 of 512 pass"""
    md = 512
    det = _blank(5, md)
    for k in range(256):
        _put(det, 0, k, 19, 24 + (k % 46) * 8, conf=_conf(k), cls=k % 3)
    _put(det, 0, 256, 208, 208, conf=0.25, cls=1)
    surv = [1]
    for t, want in ((1, 255), (2, 256), (3, 257)):
        fail = set(list(range(3, 300, 6))[:300 - want])
        assert len(fail) == 300 - want
        i = 0
        for k in range(300):
            if k in fail:
                _put(det, t, k, 397, 24 + (k % 46) * 8, conf=_conf(k), cls=k % 3)
            else:
                _put(det, t, k, *_pos(i), conf=_conf(k), cls=k % 3)
                i += 1
        surv.append(want)
    for k in range(512):
        _put(det, 4, k, *_pos(k), conf=_conf(k), cls=k % 5)
    surv.append(512)
    return _make("rounds_512", det, [257, 300, 300, 300, 512], [T416_FAR, 0, 4, 5, T416_FAR], 20, survivors=surv, kept=surv)


def _lattice_rows(n):
    """the first n boxes of gx.lattice_set(6, 4) as angle-0 det rows inside the margin: duplicates, nestings and exact IoU ties at 1/2, all of
    them integer or half-integer corners (exact in fp32)"""
    boxes, cls, conf = gx.lattice_set(6, 4, off=32)
    assert len(boxes) >= n
    rows = []
    for b, c, s in zip(boxes[:n], cls, conf):
        x0, x1, y0, y1 = min(b[0::2]), max(b[0::2]), min(b[1::2]), max(b[1::2])
        rows.append(((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0, s, c, 0.0))
    return rows


def _handover():
    """the merge's hand-over at kSegWave = 64: tiles with 63, 64, 65 and 66 survivors between empty ones (count 0, count -1, all rows outside
    the border).  md = 300."""
    md = 300
    det = _blank(8, md)
    count = [63, 0, 64, 12, 65, -1, 66, 64]
    for t in (0, 2, 4, 6, 7):
        for k, r in enumerate(_lattice_rows(count[t])):
            det[t, k] = r
    for k in range(12):
        _put(det, 3, k, 40 + 10 * k, 19)
    return _make("handover_64", det, count, [5, 0, T416_FAR, 4, 0, 5, 4, T416_FAR], 20, survivors=[63, 0, 64, 0, 65, 0, 66, 64])


def _emit():
    """k_tile_emit writes kept rows in ballot rounds of 64: tiles with 64, 65, 128 and 129 kept rows.  Disjoint boxes of mixed classes with
    exactly tied confidences (the order is fixed by stability), and after every 16th a duplicate of it (merged away: the earlier row wins
    the tie), so kept rows are not the staged rows."""
    md = 300
    want = [64, 0, 65, 128, 129, 1]
    det = _blank(6, md)
    count, surv = [], []
    for t, n in enumerate(want):
        k = 0
        for i in range(n):
            _put(det, t, k, *_pos(i), conf=0.5, cls=i % 3)
            k += 1
            if i % 16 == 5:
                _put(det, t, k, *_pos(i), conf=0.5, cls=i % 3)
                k += 1
        count.append(k), surv.append(k)
    return _make("emit_64", det, count, [5, T416_FAR, 0, 4, T416_FAR, 0], 20, survivors=surv, kept=want)


def _scan(B):
    """k_scan_counts walks B counts in rounds of 1024 with a carry.  md = 8; slot t keeps t % 9 rows: that many disjoint boxes, the rest of its
    8 rows alternately outside the border and duplicates of its first box.  Tile ids (3 t + 1) % 7: a walk over the table with repeats."""
    md = 8
    det = _blank(B, md)
    kept = []
    for t in range(B):
        n = t % 9
        for k in range(n):
            _put(det, t, k, *_pos(k), conf=_conf(k), cls=k % 2)
        for k in range(n, md):
            if n and (k - n) % 2:
                _put(det, t, k, *_pos(0), conf=0.0078125, cls=0)  # a duplicate of row 0 with a lower confidence: merged away
            else:
                _put(det, t, k, 40 + 8 * k, 9, conf=0.75, cls=0)  # outside every tile's border margin
        kept.append(n)
    tiles = [(3 * t + 1) % 7 for t in range(B)]
    # margin 10: the positions of the kept rows (24 .. 80) are inside every tile of the table but the thin one, whose slots keep nothing
    kept = [0 if tiles[t] == T_THIN else n for t, n in enumerate(kept)]
    return _make(f"scan_B{B}", det, [md] * B, tiles, 10, kept=kept)


def _capacity():
    md = 40
    det = _blank(3, md)
    for t in range(3):
        for k in range(md):
            _put(det, t, k, *_pos(k), conf=_conf(k + t), cls=k % 4)
    return _make("capacity_full", det, [md, md + 1, md], [4, 0, T416_FAR], 20, survivors=[md] * 3, kept=[md] * 3)


def _letterbox(name, lb):
    """angles just below, at and above (float)(pi / 2), negative, and beyond pi: whether the sides swap is decided by ops.results, the
    reference follows its corner bits.  12 x 6 boxes 40 px apart in the letterboxed frame (disjoint at any angle and gain 0.8); every 5th is
    followed by a copy of itself (merged away) and a copy of another class (kept); three rows lie well outside the margin."""
    h = float(HALF_PI_F)
    angs = [float(np.nextafter(HALF_PI_F, np.float32(0))), h, float(np.nextafter(HALF_PI_F, np.float32(4))), -0.3, -h, 2.0, float(PI_F), 0.7, 0.0, -3.5]
    md = 40
    det = _blank(3, md)
    count = []
    for t in range(3):
        k = 0
        for i in range(24):
            cx, cy = 60 + 40 * (i % 6), 60 + 40 * (i // 6)
            _put(det, t, k, cx, cy, 12, 6, conf=_conf(i + t), cls=i % 3, ang=angs[(i + t) % len(angs)])
            k += 1
            if i % 5 == 2:
                det[t, k] = det[t, k - 1]
                det[t, k + 1] = det[t, k - 1]
                det[t, k, 4], det[t, k + 1, 5] = 0.0078125, 7
                k += 2
        for (cx, cy) in ((6, 200), (200, 8), (330, 6)):
            _put(det, t, k, cx, cy, 12, 6, conf=0.9, cls=1, ang=angs[k % len(angs)])
            k += 1
        count.append(k)
    return _make(name, det, count, [T416_FAR, 0, 5], 20, thr=0.4, lb=lb, exact=False, survivors=[24 + 10] * 3, kept=[24 + 5] * 3)


CASES = {
    "border_416": lambda: _border("border_416", 416, 20, [T416_FAR, 0]),
    "border_128": lambda: _border("border_128", 128, 10, [T128_FAR, T128]),
    "nothing_survives": _nothing_survives,
    "margin0": _margin0,
    "counts_md1": lambda: _counts(1), "counts_md40": lambda: _counts(40), "counts_md300": lambda: _counts(300), "counts_md512": lambda: _counts(512),
    "rounds_512": _rounds,
    "handover_64": _handover,
    "emit_64": _emit,
    "scan_B1024": lambda: _scan(1024), "scan_B1025": lambda: _scan(1025), "scan_B2049": lambda: _scan(2049),
    "capacity_full": _capacity,
    "B0": lambda: _make("B0", np.zeros((0, 40, 7), np.float32), [], [], 20, survivors=[], kept=[]),
    "letterbox_gain08": lambda: _letterbox("letterbox_gain08", [[0.8, 3.0, 11.0]] * 3),
    "letterbox_none": lambda: _letterbox("letterbox_none", None),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """computed once per process and shared; callers must not modify it"""
    return CASES[name]()


def case_cls(c):
    """(int)d[5] of the rows (truncation; garbage rows give 1 000 000)"""
    return c["det"][..., 5].astype(np.int64)


def expected(c, local_pts):
    return stage(local_pts, case_cls(c), c["det"][..., 4], c["count"], c["tile_ids"], c["rects"], c["margin"], c["thr"], c["strike_cls"])


# ------------------------------------------------------------------------------------------------ strike-angle constructions (local corners)
def _quad(ax, ay, dx, dy, scale=1.0):
    """vertex 0 at (ax, ay), vertex 3 at (ax + dx, ay + dy): atan2 sees (dx, dy); vertices 1 and 2 complete a parallelogram"""
    q = [ax, ay, ax + 7.0, ay + 2.0, ax + 7.0 + dx, ay + 2.0 + dy, ax + dx, ay + dy]
    return [np.float32(v * scale) for v in q]


def angle_table():
    """-> (local_pts float32 [n, 8], cls int32 [n], tile int32 [n], names).  Every row is of class 1 or 7 (run with strike_cls 1 and 7: the rows of
    the other class must then give exactly 0.0) or of class 2 (never the strike class).
      quadrants   (dx, dy) = (+-3, +-5): atan2 in each open quadrant, away from 45 degrees (swapped arguments move it)
      axes        the eight relabellings of the integer box (100, 200)-(108, 204): the edge from vertex 0 to vertex 3 runs along +-x or +-y with an
                  exact +0.0 as the other difference: atan2 = 0, 90, 180, -90 by construction
      zeros       p6 - p0 = +0.0 (0.0 - 0.0) and -0.0 ((-0.0) - 0.0) with p7 - p1 = +-5: atan2 = +-0 and +-180 degrees; math.atan2 is the reference
      tiny        corners of 2^-60 px in the tile at x = 31 584: the global corners round them away, the local ones give 30.96 degrees"""
    rows, names = [], []
    for cls in (1, 7):
        for (dx, dy) in ((3, 5), (3, -5), (-3, -5), (-3, 5)):
            rows.append((_quad(120.0, 60.0, dx, dy), cls, T416_FAR)), names.append(f"quadrant({dx},{dy})/cls{cls}")
        for start in range(4):
            for rev in (False, True):
                rows.append(([np.float32(v) for v in gx.relabel(gx.box(100, 200, 108, 204), start, rev)], cls, (0, T128)[rev])), names.append(f"axis(start{start},rev{int(rev)})/cls{cls}")
        for z, zn in ((0.0, "+0"), (-0.0, "-0")):
            for dy in (5.0, -5.0):
                q = _quad(0.0, 50.0, 0.0, dy)
                q[6] = np.float32(z)
                rows.append((q, cls, T416_FAR)), names.append(f"zero({zn},dy{dy:+.0f})/cls{cls}")
        rows.append((_quad(1.0, 1.0, -3.0, 5.0, scale=2.0 ** -60), cls, T416_FAR)), names.append(f"tiny/cls{cls}")
    rows.append((_quad(120.0, 60.0, 3, 5), 2, 0)), names.append("another class")
    return (np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.int32), names)


def angle_expected(strike_cls, margin=20):
    lp, cls, tile, _ = angle_table()
    out = [post_row(lp[i], cls[i], RECTS[tile[i]], margin, strike_cls) for i in range(len(lp))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


def pack_rows(lp, cls, tile, conf32):
    """host-made 48-byte records of the given rows"""
    n = len(cls)
    rec = np.zeros((n, 12), np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2] = tile, cls, bits(conf32)
    rec[:, 4:] = bits(lp).reshape(n, 8)
    return rec
