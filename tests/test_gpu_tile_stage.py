"""The per-tile survivor stage on built detections against the exact reference of tile_stage_ref.py: obb_tile_survivors (k_tile_stage,
the segment merge's hand-over, k_scan_counts, k_tile_emit), the stand-alone chain obb_results -> obb_tile_postprocess -> obb_merge_segments
on the same rows, obb_records_to_dets, obb_select_kept and obb_gather_compact.  Records, tile_off, n_records, global corners, inside flags,
classes and confidences are compared bit for bit; the strike angle within the 1e-9 degrees test_gpu_geometry.py allows the device's atan2.
The local corners the reference starts from are the bits of the device's own ops.results on the same rows (tile_stage_ref.py says why).
Outputs sit between guard bands (bounds.Guarded).  Nothing here needs a model or a forward."""
import ctypes as C

import numpy as np
import pytest
import torch

import tile_stage_ref as R
from bounds import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops as o
    return o


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _raw(g):
    """a Guarded buffer's output part as it is (rows the kernel must not write keep the 0xff fill), guards checked"""
    torch.cuda.synchronize()
    assert g.guards_intact(), "write outside the output"
    return g.out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ guarded calls
def device_corners(ops, c):
    """ops.results on every row of the case (garbage rows included) -> float32 [B, md, 8]; on the `exact` cases its live rows are the host's bits"""
    B, md = c["det"].shape[:2]
    if B == 0:
        return np.zeros((0, md, 8), np.float32)
    lb = None if c["lb"] is None else dev(np.repeat(c["lb"], md, 0), torch.float32)
    pts = Guarded((B * md, 8), torch.float32)
    ops._O.results(dev(c["det"].reshape(-1, 7), torch.float32), lb, torch.empty((B * md, 5), dtype=torch.float32, device="cuda"), pts.out)
    lp = _raw(pts).reshape(B, md, 8)
    live = np.arange(md)[None, :] < c["count"][:, None]
    assert np.isfinite(lp[live]).all()
    if c["exact"]:
        assert np.array_equal(R.bits(lp[live]), R.bits(R.results_host(c["det"], None)[live])), "ops.results on angle-0 integer rows is not exact"
    return lp


def g_survivors(ops, c):
    B, md = c["det"].shape[:2]
    rec, off, n = Guarded((B * md, 12), torch.int32), Guarded((B + 1,), torch.int32), Guarded((1,), torch.int32)
    ops._O.tile_survivors(dev(c["det"], torch.float32), dev(c["count"], torch.int32), None if c["lb"] is None else dev(c["lb"], torch.float32),
                          dev(c["tile_ids"], torch.int32), dev(c["rects"], torch.int32), c["margin"], c["strike_cls"], c["thr"], rec.out, off.out, n.out)
    return _raw(rec), _raw(off), int(_raw(n)[0])


def g_post(ops, lp, cls, tile, rects, margin, strike_cls):
    n = len(cls)
    gb, ang, ins = Guarded((n, 8), torch.float64), Guarded((n,), torch.float64), Guarded((n,), torch.uint8)
    ops._O.tile_postprocess(dev(lp, torch.float32), dev(cls, torch.int32), dev(tile, torch.int32), dev(rects, torch.int32), margin, strike_cls, gb.out, ang.out, ins.out)
    return gb.get("tile_postprocess boxes").cpu().numpy(), ang.get("tile_postprocess angle").cpu().numpy(), ins.get("tile_postprocess inside").cpu().numpy()


def g_dets(ops, rec, n, rects, strike_cls):
    gb, cls, conf, ang = Guarded((n, 8), torch.float64), Guarded((n,), torch.int32), Guarded((n,), torch.float64), Guarded((n,), torch.float64)
    ops._O.records_to_dets(dev(rec, torch.int32), n, dev(rects, torch.int32), strike_cls, gb.out, cls.out, conf.out, ang.out)
    return (gb.get("records_to_dets boxes").cpu().numpy(), cls.get("records_to_dets cls").cpu().numpy(), conf.get("records_to_dets conf").cpu().numpy(),
            ang.get("records_to_dets angle").cpu().numpy())


def g_segments(ops, boxes, cls, conf, off, thr):
    n = len(boxes)
    order, keep = Guarded((n,), torch.int32), Guarded((n,), torch.uint8, init=torch.zeros(n, dtype=torch.uint8))
    ops._O.merge_segments(dev(boxes, torch.float64), dev(cls, torch.int32), dev(conf, torch.float64), dev(off, torch.int32), float(thr), order.out, keep.out)
    return order.get("segments order").cpu().numpy(), keep.get("segments keep").cpu().numpy()


# ------------------------------------------------------------------------------------------------ one stage case, everything asserted of it
_EXPECTED = {}


def expected(ops, name):
    """the reference on the device's corner bits, computed once per case and left unchanged"""
    if name not in _EXPECTED:
        c = R.case(name)
        lp = device_corners(ops, c)
        exp = R.expected(c, lp)
        assert exp["undecided"] == 0, "the exact reference must decide every pair of a committed case"
        _EXPECTED[name] = (lp, exp)
    return _EXPECTED[name]


def check_glued_chain(ops, c, lp, exp):
    """ops.results -> tile_postprocess -> merge_segments on the live rows, compacted on the host as detect._tile_records does (one segment per slot)"""
    B, md = c["det"].shape[:2]
    rows = np.nonzero((np.arange(md)[None, :] < c["count"][:, None]).reshape(-1))[0]
    if not len(rows):
        assert exp["n_records"] == 0
        return
    d, slot = c["det"].reshape(-1, 7)[rows], rows // md
    pts = Guarded((len(rows), 8), torch.float32)
    ops._O.results(dev(d, torch.float32), None if c["lb"] is None else dev(c["lb"][slot], torch.float32), torch.empty((len(rows), 5), dtype=torch.float32, device="cuda"), pts.out)
    pts = pts.get("results corners").cpu().numpy()
    assert np.array_equal(R.bits(pts), R.bits(lp.reshape(-1, 8)[rows])), "ops.results depends on where a row stands"
    cls, tile, conf32 = d[:, 5].astype(np.int32), c["tile_ids"][slot], d[:, 4]
    gb, ang, ins = g_post(ops, pts, cls, tile, c["rects"], c["margin"], c["strike_cls"])
    ref = [R.post_row(pts[i], cls[i], c["rects"][tile[i]], c["margin"], c["strike_cls"]) for i in range(len(rows))]
    R.check_post(c["name"] + " tile_postprocess", gb, ang, ins, [r[0] for r in ref], [r[1] for r in ref], [r[2] for r in ref])
    sel = np.nonzero(ins)[0]
    assert np.bincount(slot[sel], minlength=B).tolist() == exp["survivors"]
    if not len(sel):
        assert exp["n_records"] == 0
        return
    seg = np.concatenate([[0], np.cumsum(np.bincount(slot[sel], minlength=B))])
    order, keep = g_segments(ops, gb[sel], cls[sel], conf32[sel].astype(np.float64), seg, c["thr"])
    kept = sel[order[keep != 0]]
    assert np.array_equal(R.pack_rows(pts[kept], cls[kept], tile[kept], conf32[kept]), exp["records"]), "the glued chain's records differ from the reference"


def check_detections(ops, c, rec, n):
    """records_to_dets on the device's records == dets_of, and == tile_postprocess(margin 0) on the unpacked columns bit for bit"""
    if n == 0:
        return
    gb, cls, conf, ang = g_dets(ops, rec, n, c["rects"], c["strike_cls"])
    egb, ecls, econf, eang = R.dets_of(rec, n, c["rects"], c["strike_cls"])
    R.check_post(c["name"] + " records_to_dets", gb, ang, None, egb, eang)
    assert np.array_equal(cls, ecls) and np.array_equal(conf.view(np.int64), econf.view(np.int64))
    gb2, ang2, ins2 = g_post(ops, rec[:n, 4:].copy().view(np.float32), rec[:n, 1], rec[:n, 0], c["rects"], 0, c["strike_cls"])
    assert np.array_equal(gb.view(np.int64), gb2.view(np.int64)) and np.array_equal(ang.view(np.int64), ang2.view(np.int64)) and ins2.all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_stage_case(ops, name):
    c = R.case(name)
    lp, exp = expected(ops, name)
    rec, off, n = g_survivors(ops, c)
    R.check_stage(name, rec, off, n, exp)
    check_glued_chain(ops, c, lp, exp)
    check_detections(ops, c, rec, n)
    print(f"  {name}: B {c['det'].shape[0]}, md {c['det'].shape[1]}, survivors {sum(exp['survivors'])}, records {n}")


@pytest.mark.parametrize("small,large", [("border_416", "rounds_512"), ("emit_64", "scan_B2049"), ("counts_md40", "counts_md512")])
def test_a_call_after_a_larger_one_gives_equal_bits(ops, small, large):
    """the workspace slots only grow: stale staging rows of the larger call lie behind (and, across tiles, between) the live ones"""
    a = g_survivors(ops, R.case(small))
    b = g_survivors(ops, R.case(large))
    R.check_stage(large, *b, expected(ops, large)[1])
    a2 = g_survivors(ops, R.case(small))
    assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1], a2[1]) and a[2] == a2[2]
    R.check_stage(small, *a2, expected(ops, small)[1])


@pytest.mark.parametrize("n", [255, 256, 257])
def test_records_to_dets_at_the_block_edge(ops, n):
    """k_records_to_dets and k_tile_post take 256 rows per workgroup"""
    c = R.case("rounds_512")
    rec, _, total = g_survivors(ops, c)
    assert total >= 2 * 257
    check_detections(ops, c, np.ascontiguousarray(rec[300:300 + n]), n)
    gb, cls, conf, ang = g_dets(ops, rec, n, c["rects"], c["strike_cls"])  # n smaller than the buffer: the first n rows only
    assert np.array_equal(gb, R.dets_of(rec, n, c["rects"], c["strike_cls"])[0])


@pytest.mark.parametrize("strike_cls", [1, 7])
def test_strike_angle_constructions(ops, strike_cls):
    """the angle table as local corners through tile_postprocess (margins 20 and 0) and as packed rows through records_to_dets"""
    lp, cls, tile, names = R.angle_table()
    for margin in (20, 0):
        gb, ang, ins = g_post(ops, lp, cls, tile, R.RECTS, margin, strike_cls)
        for i, nm in enumerate(names):
            print(f"    {nm}: device {ang[i]!r}")
        R.check_post(f"angle table (strike {strike_cls}, margin {margin})", gb, ang, ins, *R.angle_expected(strike_cls, margin))
    conf32 = np.array([R._conf(i) for i in range(len(cls))], np.float32)
    rec = R.pack_rows(lp, cls, tile, conf32)
    gb, c2, cf, ang = g_dets(ops, rec, len(cls), R.RECTS, strike_cls)
    eg, ea, _ = R.angle_expected(strike_cls, 0)
    R.check_post(f"angle table as records (strike {strike_cls})", gb, ang, None, eg, ea)
    assert np.array_equal(c2, cls) and np.array_equal(cf, conf32.astype(np.float64))
    other = cls != strike_cls
    assert (ang[other].view(np.int64) == 0).all(), "a row of another class must give exactly +0.0"


# ------------------------------------------------------------------------------------------------ refusals
def _fill_left(*gs):
    torch.cuda.synchronize()
    return all(g.guards_intact() and bool((g.raw == 0xFF).all()) for g in gs)


@pytest.mark.parametrize("md,msg", [(0, "bad arguments"), (513, "exceeds")])
def test_max_det_outside_the_domain_is_refused(ops, md, msg):
    B = 2
    rec, off, n = Guarded((B * max(md, 1), 12), torch.int32), Guarded((B + 1,), torch.int32), Guarded((1,), torch.int32)
    det = torch.zeros((B, md, 7), dtype=torch.float32, device="cuda")
    with pytest.raises(Exception, match=msg):
        ops._O.tile_survivors(det, dev([1, 1], torch.int32), None, dev([1, 0], torch.int32), dev(R.RECTS, torch.int32), 20, 1, 0.5, rec.out, off.out, n.out)
    assert _fill_left(rec, off, n)


def test_null_buffers_are_refused(ops):
    from oriented_object_detection_amd import _lib
    c = R.case("counts_md40")
    B, md = c["det"].shape[:2]
    rec, off, n = Guarded((B * md, 12), torch.int32), Guarded((B + 1,), torch.int32), Guarded((1,), torch.int32)
    args = [dev(c["det"], torch.float32), dev(c["count"], torch.int32), dev(c["tile_ids"], torch.int32), dev(c["rects"], torch.int32), rec.out, off.out, n.out]
    for null in range(len(args)):
        p = [C.c_void_p(0) if i == null else C.c_void_p(a.data_ptr()) for i, a in enumerate(args)]
        rc = _lib.lib().obb_tile_survivors(ops.ctx(), p[0], p[1], B, md, C.c_void_p(0), p[2], p[3], 20, 1, 0.5, p[4], p[5], p[6], ops._stream())
        assert rc != 0, f"NULL argument {null} accepted"
        with pytest.raises(_lib.ObbHipError, match="NULL"):
            _lib.check(rc, ops.ctx())
        assert _fill_left(rec, off, n)
    R.check_stage("after the refusals", *g_survivors(ops, c), expected(ops, "counts_md40")[1])


# ------------------------------------------------------------------------------------------------ select_kept: k_scan_counts over block counts
def _select(ops, order, keep, n):
    """hand-made order and keep, no merge: boxes, cls, conf and angle carry their row number -> every output row names its source"""
    i = torch.arange(n, device="cuda")
    boxes = (i.double()[:, None] * 8 + torch.arange(8, device="cuda").double()[None, :]).contiguous()
    cls, conf, ang = i.int(), i.double() + 0.5, -i.double()
    ob, oc, of, oa, cnt = (Guarded((n, 8), torch.float64), Guarded((n,), torch.int32), Guarded((n,), torch.float64), Guarded((n,), torch.float64), Guarded((1,), torch.int32))
    ops._O.select_kept(order, keep, boxes, cls, conf, ang, ob.out, oc.out, of.out, oa.out, cnt.out)
    torch.cuda.synchronize()
    src = order[keep.bool()].long()
    m = int(cnt.out[0])
    assert m == src.numel()
    for g in (ob, oc, of, oa, cnt):
        assert g.guards_intact()
    assert torch.equal(ob.out[:m], boxes[src]) and torch.equal(oc.out[:m], cls[src]) and torch.equal(of.out[:m], conf[src]) and torch.equal(oa.out[:m], ang[src])
    for g in (ob, oc, of, oa):  # rows at and past the count keep the fill
        assert bool((g.out[m:].contiguous().view(-1).view(torch.uint8) == 0xFF).all())
    return m


def test_select_kept_scans_more_than_1024_blocks(ops):
    """n = 1024 * 1024 + 1: 1025 block counts, the second round of k_scan_counts carries the first's total.  Every 3rd position kept."""
    n = 1024 * 1024 + 1
    i = torch.arange(n, device="cuda")
    order = ((i * 7 + 5) % n).int()  # a permutation (n = 17 * 61681)
    keep = (i % 3 == 0).to(torch.uint8)
    assert _select(ops, order, keep, n) == (n + 2) // 3


@pytest.mark.parametrize("fill", [0, 1])
def test_select_kept_all_or_nothing(ops, fill):
    n = 1025
    order = torch.arange(n - 1, -1, -1, device="cuda").int()
    assert _select(ops, order, torch.full((n,), fill, dtype=torch.uint8, device="cuda"), n) == fill * n


# ------------------------------------------------------------------------------------------------ gather_compact
@pytest.mark.parametrize("world", [1, 8])
@pytest.mark.parametrize("cap", [1, 300])
def test_gather_compact_at_the_capacity(ops, world, cap):
    """counts 0, equal to the capacity and above it, on the first and on the last rank; against the slicing test_gather_compact uses"""
    rng = np.random.default_rng(world * 1000 + cap)
    for first, last in ((0, cap + 5), (cap, 0), (cap + 1, cap), (0, 0), (cap, cap)):
        counts = [int(v) for v in rng.integers(0, cap + 1, world)]
        counts[0], counts[-1] = first, last
        recv = rng.integers(-2 ** 31, 2 ** 31 - 1, (world, cap + 1, 12), dtype=np.int64).astype(np.int32)
        recv[:, 0, 0] = counts
        out, cnt = Guarded((world * cap, 12), torch.int32), Guarded((world + 1,), torch.int32)
        ops._O.gather_compact(dev(recv, torch.int32), out.out, cnt.out)
        rows, got = _raw(out), _raw(cnt).tolist()
        exp = np.concatenate([recv[r, 1:1 + min(c, cap)] for r, c in enumerate(counts)], 0)
        assert got[:world] == counts and got[world] == len(exp), (counts, got)
        assert np.array_equal(rows[:len(exp)], exp) and bool((rows[len(exp):] == R.FILL).all())
