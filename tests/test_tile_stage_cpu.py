"""The cases of tile_stage_ref.py satisfy their own conditions, and the checker of test_gpu_tile_stage.py catches a wrong stage (no GPU).

The stand-in below is the per-tile survivor stage in numpy with the structure of the kernels (csrc/geom.hip): staging in rounds of 256 rows
with a carry, a merge hand-over at 64 survivors, emit rounds of 64, a scan in rounds of 1024 with a carry.  Run unplanted, it passes the
checker on every case.  Each plant fails the checker on the cases named in PLANTS:

  lt_low        `<` for `<=` at the low end of the border test      border_416, border_128 (centres at m)
  lt_high       `<` for `<=` at the high end                         border_416, border_128 (centres at size - m)
  skip_x        the margin test skipped for x                        border_416, border_128 (rows that fail x only)
  skip_y        the margin test skipped for y                        border_416, border_128, nothing_survives (the 10-px crop)
  angle_global  the angle taken from the global corners              the angle table (signed-zero rows at an offset, the 2^-60 px rows)
  ge_branch     `180 - a` applied for a >= 0                         the angle table (atan2 = +0 and -0 rows)
  round_carry   the carry dropped in the 256-row compaction          rounds_512, counts_md512
  emit_base     the emit base not advanced after a round of 64       emit_64, handover_64
  scan_carry    the scan carry dropped after 1024                    scan_B1025, scan_B2049
  no_clamp      count not clamped to max_det                         counts_md40, counts_md1
  tile_slot     the record's tile id taken as the slot index         border_416, scan_B1024"""
import math

import numpy as np
import pytest

import tile_stage_ref as R

STAGE_CASES = tuple(R.CASES)


# ------------------------------------------------------------------------------------------------ the stand-in
def _post(lp, cls, rect, margin, strike_cls, plant=None):
    """tile_post_row over the rows of one round (numpy float64: the same IEEE operations per element) -> (g [n, 8], angle [n], inside [n])"""
    x, y, x2, y2 = (int(v) for v in rect)
    p = np.asarray(lp, np.float32).reshape(-1, 8).astype(np.float64)
    g = p + np.array([x, y] * 4, np.float64)
    with np.errstate(invalid="ignore"):
        cx, cy = (g[:, 0] + g[:, 2] + g[:, 4] + g[:, 6]) / 4.0, (g[:, 1] + g[:, 3] + g[:, 5] + g[:, 7]) / 4.0
        cxr, cyr, m, cw, ch = cx - x, cy - y, float(margin), float(x2 - x), float(y2 - y)
        lo = (lambda c: m < c) if plant == "lt_low" else (lambda c: m <= c)
        hi = (lambda c, s: c < s - m) if plant == "lt_high" else (lambda c, s: c <= s - m)
        okx = np.ones(len(p), bool) if plant == "skip_x" else lo(cxr) & hi(cxr, cw)
        oky = np.ones(len(p), bool) if plant == "skip_y" else lo(cyr) & hi(cyr, ch)
        ins = okx & oky if margin > 0 else np.ones(len(p), bool)
        q = g if plant == "angle_global" else p
        a = np.arctan2(q[:, 6] - q[:, 0], q[:, 7] - q[:, 1]) * R.K_DEG
        a = np.where((a >= 0) if plant == "ge_branch" else (a > 0), 180 - a, np.abs(a))
    return g, np.where(np.asarray(cls) == strike_cls, a, 0.0), ins


def standin_post(lp, cls, tile, rects, margin, strike_cls, plant=None):
    """k_tile_post / k_records_to_dets: rows of mixed tiles"""
    n = len(cls)
    g, a, ins = np.zeros((n, 8)), np.zeros(n), np.zeros(n, bool)
    for i in range(n):
        g[i], a[i], ins[i] = (v[0] for v in _post(lp[i], [cls[i]], rects[tile[i]], margin, strike_cls, plant))
    return g, a, ins


def standin_stage(c, lp, plant=None):
    """obb_tile_survivors -> (records [B * md, 12] with the guard fill behind n, tile_off [B + 1], n_records)"""
    det, count, tile_ids, rects = c["det"], c["count"], c["tile_ids"], c["rects"]
    B, md = det.shape[:2]
    cap, pad = B * md, 16 + md  # (an unclamped count walks off its tile: rows and slots behind the arrays, as garbage)
    if B == 0:
        return np.full((0, 12), R.FILL, np.int32), np.full(1, R.FILL, np.int32), 0
    flat_lp = np.concatenate([np.asarray(lp, np.float32).reshape(cap, 8), np.full((pad, 8), np.nan, np.float32)])
    flat_cls = np.concatenate([R.case_cls(c).reshape(cap), np.full(pad, 10 ** 6)])
    flat_cf = np.concatenate([det[..., 4].reshape(cap), np.full(pad, 2.0, np.float32)]).astype(np.float32)
    S_gb, S_cls, S_cf, S_pts = np.zeros((cap + pad, 8)), np.full(cap + pad, -7), np.zeros(cap + pad, np.float32), np.zeros((cap + pad, 8), np.float32)  # stale staging rows
    lo, hi = np.zeros(B, int), np.zeros(B, int)
    for t in range(B):  # k_tile_stage: one workgroup per tile, rounds of 256 rows, ordered compaction with a carry
        n = int(count[t]) if plant == "no_clamp" else min(int(count[t]), md)
        base = 0
        for k0 in range(0, n, 256):
            rows = t * md + np.arange(k0, min(k0 + 256, n))
            g, _, ins = _post(flat_lp[rows], flat_cls[rows], rects[tile_ids[t]], c["margin"], c["strike_cls"], plant)
            sel = np.nonzero(ins)[0]
            slot = t * md + (0 if plant == "round_carry" else base) + np.arange(len(sel))
            S_gb[slot], S_cls[slot], S_cf[slot], S_pts[slot] = g[sel], flat_cls[rows][sel], flat_cf[rows][sel], flat_lp[rows][sel]
            base += len(sel)
        lo[t], hi[t] = t * md, t * md + base
    order, keep, nkeep = np.zeros(cap + pad, int), np.zeros(cap + pad, np.uint8), np.zeros(B, int)

    def merge_seg(t):
        s = slice(lo[t], hi[t])
        (o, k), _ = R.merge(S_gb[s], S_cls[s], S_cf[s].astype(np.float64), c["thr"])
        order[s], keep[s], nkeep[t] = lo[t] + np.array(o, int), np.array(k, np.uint8), sum(k)
    long_list = []
    for t in range(B):  # k_merge_segments_wave: up to kSegWave = 64 rows; the rest go on the list
        long_list.append(t) if hi[t] - lo[t] > 64 else merge_seg(t)
    for t in long_list:  # k_merge_segments, from the list
        merge_seg(t)
    off, carry = np.zeros(B + 1, np.int32), 0
    for i0 in range(0, B, 1024):  # k_scan_counts: rounds of 1024 with a carry
        v = nkeep[i0:i0 + 1024]
        incl = np.cumsum(v)
        off[i0:i0 + len(v)] = (0 if plant == "scan_carry" else carry) + incl - v
        carry += int(incl[-1])
    off[B] = carry
    rec = np.full((cap, 12), R.FILL, np.int32)
    for t in range(B):  # k_tile_emit: one wave per tile, ballot rounds of 64
        base = int(off[t])
        for i0 in range(0, hi[t] - lo[t], 64):
            i = lo[t] + np.arange(i0, min(i0 + 64, hi[t] - lo[t]))
            src = order[i[keep[i] != 0]]
            dst = base + np.arange(len(src))
            src, dst = src[dst < cap], dst[dst < cap]
            rec[dst, 0], rec[dst, 1], rec[dst, 2], rec[dst, 3] = (t if plant == "tile_slot" else tile_ids[t]), S_cls[src], R.bits(S_cf[src]), 0
            rec[dst, 4:] = R.bits(S_pts[src]).reshape(-1, 8)
            if plant != "emit_base":
                base += len(src)
    return rec, off, int(off[B])


def run_stage(name, plant=None):
    """the stand-in through everything the GPU test asserts of the device on a stage case"""
    c = R.case(name)
    lp = R.results_host(c["det"], c["lb"])
    exp = R.expected(c, lp)
    rec, off, n = standin_stage(c, lp, plant)
    R.check_stage(name, rec, off, n, exp)
    gb, cls, conf, ang = R.dets_of(exp["records"], exp["n_records"], c["rects"], c["strike_cls"])
    r = exp["records"]
    g2, a2, _ = standin_post(r[:, 4:].copy().view(np.float32), r[:, 1], r[:, 0], c["rects"], 0, c["strike_cls"], plant)
    R.check_post(name + " detections", g2, a2, None, gb, ang)
    return exp


def run_angles(strike_cls, plant=None):
    lp, cls, tile, _ = R.angle_table()
    for margin in (20, 0):
        g, a, ins = standin_post(lp, cls, tile, R.RECTS, margin, strike_cls, plant)
        R.check_post(f"angle table (strike {strike_cls}, margin {margin})", g, a, ins, *R.angle_expected(strike_cls, margin))


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", STAGE_CASES)
def test_case_is_decided_and_as_promised_and_the_standin_passes(name):
    """0 undecided pairs; the survivor and kept counts the case names promise; every border centre the intended integer; every row past a
    count is garbage; the unplanted stand-in passes the checker"""
    c = R.case(name)
    exp = run_stage(name)
    assert exp["undecided"] == 0, "the exact reference must decide every pair of a committed case"
    if c["survivors"] is not None:
        assert exp["survivors"] == c["survivors"], (exp["survivors"], c["survivors"])
    if c["kept"] is not None:
        assert exp["kept"] == c["kept"], (exp["kept"], c["kept"])
    B, md = c["det"].shape[:2]
    lp = R.results_host(c["det"], c["lb"])
    for (t, k, cx, cy) in c["centres"]:
        rect = c["rects"][c["tile_ids"][t]]
        assert all(float(v) == int(v) for v in lp[t, k])  # integer corners
        g, _, _ = R.post_row(lp[t, k], 0, rect, c["margin"], 1)
        assert (g[0] + g[2] + g[4] + g[6]) / 4.0 - float(rect[0]) == cx and (g[1] + g[3] + g[5] + g[7]) / 4.0 - float(rect[1]) == cy
    if name.startswith("border"):
        assert len(c["centres"]) == B * 19 and 0 < exp["survivors"][0] < 19
    for t in range(B):
        live = max(0, min(int(c["count"][t]), md))
        assert np.isnan(c["det"][t, live:, :4]).all() and (c["det"][t, live:, 4] == 2.0).all() and (c["det"][t, live:, 5] == 1e6).all()
        assert np.isfinite(c["det"][t, :live]).all()
    if B:
        assert (c["tile_ids"] != np.arange(B)).any(), "tile ids equal to the slot indices hide a swapped one"
    if c["exact"]:
        live = np.arange(md)[None, :] < c["count"][:, None]
        assert (c["lb"] is None) and np.isin(c["det"][..., 6][live], (0.0, float(R.HALF_PI_F))).all()


def test_case_shapes_reach_the_paths_they_name():
    e = {n: R.expected(R.case(n), R.results_host(R.case(n)["det"], R.case(n)["lb"])) for n in ("rounds_512", "handover_64", "emit_64", "capacity_full", "scan_B2049")}
    assert e["rounds_512"]["survivors"] == [1, 255, 256, 257, 512] and list(R.case("rounds_512")["count"]) == [257, 300, 300, 300, 512]
    h = e["handover_64"]
    assert h["survivors"] == [63, 0, 64, 0, 65, 0, 66, 64] and all(k < s for k, s in zip(h["kept"], h["survivors"]) if s), "some rows must be merged away"
    assert e["emit_64"]["kept"] == [64, 0, 65, 128, 129, 1] and all(s > k for s, k in zip(e["emit_64"]["survivors"][2:5], e["emit_64"]["kept"][2:5]))
    assert e["capacity_full"]["n_records"] == 3 * 40
    k = e["scan_B2049"]["kept"]
    assert set(k) == set(range(9)) and len(k) == 2049 and k[1024] > 0 and k[2048] > 0  # the later rounds of the scan carry rows
    assert len(set(R.case("scan_B2049")["tile_ids"].tolist())) == 7  # a walk with repeats
    for md in (1, 40, 300, 512):
        assert list(R.case(f"counts_md{md}")["count"]) == [-3, 0, md + 7, md, 1]


def _rule(dx, dy, how):
    a = math.atan2(dx, dy) * R.K_DEG
    if how == "branch":
        return abs(a) if a > 0 else 180 - a
    if how == "ge":
        return 180 - a if a >= 0 else abs(a)
    return 180 - a if a > 0 else abs(a)


@pytest.mark.parametrize("strike_cls", [1, 7])
def test_angle_cases_are_separated_from_every_wrong_rule(strike_cls):
    """each row of the angle table is at least ANGLE_SEP degrees from what one of the wrong rules gives, and each wrong rule moves some row:
    the other branch, the sign of the first argument, global for local corners, swapped arguments, `>=` for `>`, the rule for every class"""
    lp, cls, tile, names = R.angle_table()
    _, ref, _ = R.angle_expected(strike_cls)
    caught = {k: 0 for k in ("branch", "sign", "global", "swapped", "ge", "every class")}
    for i, name in enumerate(names):
        p = [float(v) for v in lp[i]]
        x, y = float(R.RECTS[tile[i]][0]), float(R.RECTS[tile[i]][1])
        dx, dy = p[6] - p[0], p[7] - p[1]
        wrong = {"every class": _rule(dx, dy, "ok")} if cls[i] != strike_cls else {
            "branch": _rule(dx, dy, "branch"), "sign": _rule(p[0] - p[6], dy, "ok"), "global": _rule((p[6] + x) - (p[0] + x), (p[7] + y) - (p[1] + y), "ok"),
            "swapped": _rule(dy, dx, "ok"), "ge": _rule(dx, dy, "ge")}
        moved = {k: abs(v - ref[i]) for k, v in wrong.items()}
        for k, v in moved.items():
            caught[k] += v >= R.ANGLE_SEP
        if cls[i] != strike_cls:  # a row of another class: exactly +0.0 (the strike rule itself gives 0 on two of the axes: those rows cannot tell)
            assert ref[i] == 0.0 and math.copysign(1.0, ref[i]) == 1.0
            assert name != "another class" or moved["every class"] >= R.ANGLE_SEP
        else:
            assert max(moved.values()) >= R.ANGLE_SEP, (name, moved)
    assert all(caught.values()), caught
    zeros = {n: ref[i] for i, n in enumerate(names) if n.startswith("zero") and n.endswith(f"cls{strike_cls}")}
    got = [zeros[f"zero({z},dy{d})/cls{strike_cls}"] for z in ("+0", "-0") for d in ("+5", "-5")]  # math.atan2 on the signed zeros: 0, 180, -0, -180 degrees
    assert np.allclose(got, [0.0, 0.0, 0.0, 180.0], rtol=0, atol=1e-12), got
    run_angles(strike_cls)


# ------------------------------------------------------------------------------------------------ the plants
PLANTS = {
    "lt_low": ("border_416", "border_128"), "lt_high": ("border_416", "border_128"), "skip_x": ("border_416", "border_128"),
    "skip_y": ("border_416", "border_128", "nothing_survives"), "angle_global": ("angles",), "ge_branch": ("angles",),
    "round_carry": ("rounds_512", "counts_md512"), "emit_base": ("emit_64", "handover_64"), "scan_carry": ("scan_B1025", "scan_B2049"),
    "no_clamp": ("counts_md40", "counts_md1"), "tile_slot": ("border_416", "scan_B1024"),
}


@pytest.mark.parametrize("plant", list(PLANTS))
def test_every_plant_fails_its_named_cases(plant):
    for name in PLANTS[plant]:
        with pytest.raises(AssertionError):
            if name == "angles":
                run_angles(1, plant)
            else:
                run_stage(name, plant)
        if name == "angles":
            with pytest.raises(AssertionError):
                run_angles(7, plant)
