"""The batch and validation kernels (k_aug_tiles, k_aug_labels, k_val_match) at their launch and domain edges, against tests/aug_ref.py (numpy / fp64,
materialised canvas) and tests/val_ref.py (fp64), with the yardsticks of test_gpu_augment.py and test_gpu_validate.py unchanged: pixels bit for bit;
label counts, classes, masks and order exact and every box element within `box_tol`; `tp` and `best_gt` exact and `best_iou` within the band
(4 x max |fp32 - fp64| of every candidate pair of every committed case, evaluated by the reference on the CPU: val_ref.all_band()).  The cases come
from aug_ref.label_edge_cases() and val_ref.edge_cases(); tests/test_augment_cpu.py and tests/test_validate_cpu.py assert on the CPU that they
keep clear of every discrete decision and hold what they claim (which prefix-sum passes hold survivors, which detections share a lane)."""
import numpy as np
import pytest
import torch

import aug_ref as R
import test_gpu_augment as TA
import val_ref as VR
from bounds import Guarded

pytestmark = pytest.mark.gpu

SRC = (3, 0, 6, 1)


def _run_pixels(A, ops, pool, dpool, table, bgr=True, swap=False):
    """ops.aug_tiles into a guarded buffer == tiles_ref, byte for byte -> the device's tiles"""
    B, s, C = len(table), pool.shape[1], pool.shape[3]
    exp = R.tiles_ref(pool, table, bgr, swap)
    big, out = TA._guarded(B, s, C)
    got = ops.aug_tiles(dpool, TA._dev_table(A, table), bgr, swap, out=out).cpu().numpy()
    bad = np.argwhere(got != exp)
    assert np.array_equal(got, exp), (B, s, C, bgr, swap, len(bad), bad[:4].tolist(), [(int(got[tuple(i)]), int(exp[tuple(i)])) for i in bad[:4]])
    assert bool((big[0] == 0xAB).all()) and bool((big[-1] == 0xAB).all())
    return got


# ---------------------------------------------------------------- pixels
@pytest.mark.parametrize("mosaic", [True, False], ids=["mosaic", "single"])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("s", [2, 3, 7, 9, 33, 36, 50, 100])
def test_pixel_sides(s, C, mosaic):
    """sides that are no multiple of the strip of 8 rows (the last strip has s % 8 rows; under 8 the only one is short; under 32 a strip has fewer
    pixels than lanes), each of pixel_tables' five variants at B = 1 and all of them over two tables of B = 3"""
    _, A, ops, _, _ = TA._mods()
    pool = R.random_pool(7, s, C, seed=s + C)
    dpool = torch.from_numpy(pool).cuda()
    modes = [(True, False), (True, True), (False, True)]
    for k, (B, seed) in enumerate([(3, 0), (3, 3), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4)]):
        _run_pixels(A, ops, pool, dpool, R.pixel_tables(7, s, B, mosaic, seed), *modes[k % 3])


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("centre", R.centre_ends(36), ids=lambda c: f"{c[0]}-{c[1]}")
def test_pixel_centres_at_the_ends(centre, C):
    """a mosaic centre at 0 or 2 s: one or two quadrants are empty and the tap arithmetic has to agree with the materialised canvas, with all of the
    canvas in view (scale 0.5) and at the identity scale"""
    _, A, ops, _, _ = TA._mods()
    s = 36
    pool = R.random_pool(7, s, C, seed=50 + C)
    dpool = torch.from_numpy(pool).cuda()
    table = R.centre_table(s, centre, SRC)
    cv = R.canvas_of(pool, table[0])
    assert (cv == R.BORDER).all(-1).mean() >= 0.5  # at least two of the four quadrants are empty
    got = _run_pixels(A, ops, pool, dpool, table)
    for b in range(3):
        assert np.array_equal(_run_pixels(A, ops, pool, dpool, table[b:b + 1], True, b == 1)[0][..., 1], got[b][..., 1])
    assert (got[0] != got[0][0, 0]).any() and (got[1] != got[1][0, 0]).any()  # something of the pool is in view in both


@pytest.mark.parametrize("mosaic", [True, False], ids=["mosaic", "single"])
@pytest.mark.parametrize("C", [3, 4])
def test_pixel_maps_that_leave_the_canvas(C, mosaic):
    _, A, ops, _, _ = TA._mods()
    s = 36
    pool = R.random_pool(7, s, C, seed=60 + C)
    pool[:, 0, 0] = 200  # canvas(0, 0) is not the border value
    dpool = torch.from_numpy(pool).cuda()
    for hsv in (False, True):
        table = R.offcanvas_table(7, s, mosaic, hsv, seed=C)
        got = _run_pixels(A, ops, pool, dpool, table[:R.OFF_BORDER])
        grey = np.full((1, 1, 3), R.BORDER, np.uint8)
        after = R.hsv_apply(grey.copy(), table[0]["lut"]) if hsv else grey
        assert (got[..., :3] == after).all() and (hsv or (got == R.BORDER).all())
        one = _run_pixels(A, ops, pool, dpool, table[R.OFF_BORDER:])[0]
        if not hsv:  # the two saturated terms cancel: canvas(0, 0) wherever x, y >= 1 (and at the origin), the border on the rest of row and column 0
            assert (one[1:, 1:] == 200).all() and (one[0, 0] == 200).all() and (one[0, 1:] == R.BORDER).all() and (one[1:, 0] == R.BORDER).all()


@pytest.mark.parametrize("C", [3, 4])
def test_pixel_batch_limit(C):
    """65535 tiles in one call run (the grid's second dimension at its limit); 65536 are refused and nothing is written"""
    lib, A, ops, _, _ = TA._mods()
    pool = R.random_pool(3, 2, C, seed=70)
    dpool = torch.from_numpy(pool).cuda()
    table = torch.zeros((65536, A.REC.itemsize), dtype=torch.uint8, device="cuda")  # all-zero records: no flags, source 0, the zero map: canvas(0, 0)
    big = torch.full((65536 + 2, 2, 2, C), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(lib.ObbHipError):
        ops.aug_tiles(dpool, table, True, False, out=big[1:65537])
    torch.cuda.synchronize()
    assert bool((big == 0xAB).all())
    out = ops.aug_tiles(dpool, table[:65535], True, False, out=big[1:65536])
    exp = R.tiles_ref(pool, np.zeros(1, A.REC))[0]
    assert (exp == pool[0, 0, 0]).all() and bool((out == torch.from_numpy(exp).cuda()[None]).all())
    assert bool((big[0] == 0xAB).all()) and bool((big[65536:] == 0xAB).all())


@pytest.fixture(scope="module")
def colours():
    pool = R.colour_pool()
    return pool, torch.from_numpy(pool).cuda()


def _compare_colours(got, exp, src, what):
    bad = np.argwhere((got != exp).any(-1))
    first = [(tuple(int(v) for v in src[tuple(i)][:3]), got[tuple(i)].tolist(), exp[tuple(i)].tolist()) for i in bad[:5]]
    assert not len(bad), f"{what}: {len(bad)} colours differ; first (b, g, r), got, expected: {first}"


@pytest.mark.parametrize("gains", [(1.0, 1.0, 1.0), (0.985, 0.3, 0.6), (1.015, 1.7, 1.4), R.HUE_LUT_OUT_OF_RANGE], ids=str)
def test_colour_domain(colours, gains):
    """every one of the 2^24 colours through the HSV round trip (integer BGR -> HSV, three tables, fp32 HSV -> BGR): one product or sum contracted
    into a fused multiply-add on the device would show as single colours off by one"""
    _, A, ops, _, _ = TA._mods()
    pool, dpool = colours
    table = R.colour_table(gains)
    if isinstance(gains, str):
        assert table[0]["lut"][:180].max() == 255 and (table[0]["lut"][:180] >= 180).sum() == 76 and 180 in table[0]["lut"][:180]
    big, out = TA._guarded(16, 1024, 3)
    got = ops.aug_tiles(dpool, TA._dev_table(A, table), True, False, out=out).cpu().numpy()
    assert bool((big[0] == 0xAB).all()) and bool((big[-1] == 0xAB).all())
    for t in range(16):
        _compare_colours(got[t], R.hsv_apply(pool[t].copy(), table[t]["lut"]), pool[t], f"gains {gains}, tile {t}")


def test_colour_domain_channel_orders(colours):
    """one tile of the colour pool read as RGB and written swapped, and one with a fourth channel, which passes through"""
    _, A, ops, _, _ = TA._mods()
    pool, dpool = colours
    table = R.colour_table((1.015, 1.7, 0.6), tiles=[11])
    got = ops.aug_tiles(dpool, TA._dev_table(A, table), False, True).cpu().numpy()[0]
    exp = R.hsv_apply(pool[11].copy(), table[0]["lut"], bgr=False)[..., ::-1]
    _compare_colours(got, exp, pool[11], "bgr=False, swap_rb=True")
    four = np.concatenate([pool[6], np.random.RandomState(4).randint(0, 256, (1024, 1024, 1)).astype(np.uint8)], -1)[None]
    table = R.colour_table((0.985, 1.7, 1.4), tiles=[0])
    big, out = TA._guarded(1, 1024, 4)
    got = ops.aug_tiles(torch.from_numpy(four).cuda(), TA._dev_table(A, table), True, False, out=out).cpu().numpy()[0]
    assert bool((big[0] == 0xAB).all()) and bool((big[-1] == 0xAB).all())
    _compare_colours(got, R.hsv_apply(four[0].copy(), table[0]["lut"]), four[0], "C = 4")
    assert np.array_equal(got[..., 3], four[0][..., 3])


# ---------------------------------------------------------------- labels
@pytest.mark.parametrize("case", R.label_edge_cases(), ids=lambda c: c[0])
def test_label_edges(case):
    _, A, ops, _, _ = TA._mods()
    name, s, lab, cnt, table, n_cap = case
    exp = R.labels_ref(lab, cnt, table, s, n_cap)
    got = TA._run_labels(A, ops, s, lab, cnt, table, n_cap)
    TA._check_labels(got, exp, s, name)
    again = TA._run_labels(A, ops, s, lab, cnt, table, n_cap)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))  # bit-identical on repeat
    gl, gb, mk, ct = got
    live = np.arange(n_cap)[None, :] < np.minimum(ct, n_cap)[:, None]
    assert np.array_equal(mk, live)  # the survivors first, every row behind them unmasked -- and zero (_check_labels)
    if name.endswith(("inside", "boundary")) or name == "few-n_cap1":
        assert (ct > n_cap).any()
    if name == "Lmax0":
        assert lab.shape[1] == 0 and not ct.any() and not mk.any() and not gl.any() and not gb.any()
    if name == "counts-outside":
        assert ct[:2].min() > 0


# ---------------------------------------------------------------- matching
def _match_on_device(ops, case):
    det, count, gl, gb, mk, nc, thr = case[:7]
    B, M = det.shape[:2]
    outs = (Guarded((B, M), torch.uint16, init=None), Guarded((B, M), torch.float32), Guarded((B, M), torch.int32))
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (det, count, gl, gb, mk)]
    ops.val_match(*d, nc, thr=torch.from_numpy(thr).cuda(), out=tuple(g.out for g in outs))
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in outs)
    return tuple(g.out.cpu().numpy() for g in outs)


@pytest.mark.parametrize("case", VR.edge_cases(), ids=lambda c: c[7])
def test_val_match_edges(case):
    _, _, ops, _, _ = TA._mods()
    name = case[7]
    band, _ = VR.all_band()
    ref_tp, ref_bi, ref_bg = VR.match(*case[:6], thr=case[6])
    tp, bi, bg = _match_on_device(ops, case)
    assert np.array_equal(bg, ref_bg), np.argwhere(bg != ref_bg)[:8]
    assert np.array_equal(tp, ref_tp), np.argwhere(tp != ref_tp)[:8]
    print(f"val_match {name}: max |best_iou - fp64| = {np.abs(bi - ref_bi).max():.3e}, band {band:.3e}")
    assert np.abs(bi.astype(np.float64) - ref_bi).max() <= band
    VR.edge_claims(case, tp, bi, bg)
    other = {"invalid-rows": lambda: VR.invalid_case(VR.EDGE_SEEDS["invalid"], bad=False), "counts": lambda: VR.counts_case(VR.EDGE_SEEDS["counts"], clamped=True)}
    if name in other:  # the same data without the invalid rows / with the counts already clamped: every row's result is the same, bit for bit
        again = _match_on_device(ops, other[name]())
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((tp, bi, bg), again))


def test_val_match_no_images():
    """B = 0 returns without touching the outputs"""
    lib, _, ops, _, _ = TA._mods()
    dev = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    tp, bi, bg = ops.val_match(dev((0, 5, 7), torch.float32), dev((0,), torch.int32), dev((0, 4), torch.int32), dev((0, 4, 5), torch.float32), dev((0, 4), torch.bool), 3)
    assert tp.shape == bi.shape == bg.shape == (0, 5)
    outs = (Guarded((2, 5), torch.uint16, init=None), Guarded((2, 5), torch.float32), Guarded((2, 5), torch.int32))
    d = [dev((2, 5, 7), torch.float32), torch.full((2,), 5, dtype=torch.int32, device="cuda"), dev((2, 4), torch.int32), dev((2, 4, 5), torch.float32), dev((2, 4), torch.uint8)]
    thr = ops.val_thresholds("cuda")
    args = [ops._p(t) for t in d] + [0, 5, 4, 3, ops._p(thr), 10] + [ops._p(g.out) for g in outs] + [ops._stream()]
    assert lib.lib().obb_val_match(ops.ctx(), *args) == 0
    torch.cuda.synchronize()
    assert all(bool((g.raw == 0xFF).all()) for g in outs)
