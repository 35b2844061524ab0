"""f1 (training batches) on the device against tests/aug_ref.py: the pixel kernel bit for bit (the reference materialises the mosaic canvas and warps
it whole; the kernel gathers every tap through the quadrant arithmetic), the label kernel with identical counts, classes, masks and order and every
box element within BOX_TOL, the capture of a whole batch, and a batch from the tiler's pool through `Net.forward_backward`.

BOX_TOL(ref, s) = one fp32 ulp of max(|ref|, 1) + 1e-12 s.  The first term is the output's own format (the device rounds its fp64 result to fp32 once:
half an ulp; the other half covers a reference that sits next to a rounding boundary).  The second is the fp64 path, derived, not fitted: a coordinate
goes through at most 40 fp64 operations (scale and pad 2, the affine map 5, a flip 1, one clip interpolation per side 5 each but at most two sides
touch one vertex, two projections 3 each, extents 2, the centre 6) on magnitudes up to 4 s (the canvas is 2 s wide, |M| <= 1.5 plus translation), so
it is off by at most 40 * 2^-53 * 4 s = 1.8e-14 s in either implementation, 3.6e-14 s between the two; theta comes from an edge of at least one pixel
whose end points carry that error: 2 * 3.6e-14 s rad.  Both are under 1e-12 s with more than a factor of ten to spare."""
import math

import numpy as np
import pytest
import torch

import aug_ref as R

pytestmark = pytest.mark.gpu


def _mods():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, augment, ops, tiler, train
    return _lib, augment, ops, tiler, train


def _dev_table(A, table):
    return A.table_to_device(table, "cuda")


def box_tol(ref, s):
    return np.spacing(np.maximum(np.abs(ref), 1.0).astype(np.float32)).astype(np.float64) + 1e-12 * s


def _guarded(B, s, C):
    big = torch.full((B + 2, s, s, C), 0xAB, dtype=torch.uint8, device="cuda")
    return big, big[1:B + 1]


# ---------------------------------------------------------------- pixels
@pytest.mark.parametrize("mosaic", [True, False], ids=["mosaic", "single"])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("s", [32, 40, 64])
def test_pixels_bit_for_bit(s, C, mosaic):
    _, A, ops, _, _ = _mods()
    pool = R.random_pool(7, s, C, seed=s + C)
    dpool = torch.from_numpy(pool).cuda()
    for B in (1, 5):
        for seed, (bgr, swap) in enumerate([(True, False), (True, True), (False, True)]):
            table = R.pixel_tables(7, s, B, mosaic, seed + B)
            exp = R.tiles_ref(pool, table, bgr, swap)
            big, out = _guarded(B, s, C)
            got = ops.aug_tiles(dpool, _dev_table(A, table), bgr, swap, out=out)
            assert got.data_ptr() == out.data_ptr()
            got = got.cpu().numpy()
            bad = np.argwhere(got != exp)
            assert np.array_equal(got, exp), (B, bgr, swap, len(bad), bad[:4].tolist(), [(int(got[tuple(i)]), int(exp[tuple(i)])) for i in bad[:4]])
            assert bool((big[0] == 0xAB).all()) and bool((big[-1] == 0xAB).all())


def test_pixels_sampled_params_and_identity():
    """what `sample_params` draws with the default configuration (HSV gains in the open range, fractional translations), and the identity record"""
    _, A, ops, _, _ = _mods()
    s = 40
    pool = R.random_pool(7, s, 3, seed=11)
    dpool = torch.from_numpy(pool).cuda()
    table = A.sample_params(A.AugmentConfig(degrees=5.0, flipud=0.5), 5, 7, s, np.random.RandomState(3))
    assert np.array_equal(ops.aug_tiles(dpool, _dev_table(A, table), True, True).cpu().numpy(), R.tiles_ref(pool, table, True, True))
    ident = np.zeros(1, A.REC)
    A.make_record(ident[0], np.eye(3), 1.0, s, src=(5, 0, 0, 0))
    assert np.array_equal(ops.aug_tiles(dpool, _dev_table(A, ident), True, False).cpu().numpy()[0], pool[5])


def test_refusals_write_nothing():
    lib, A, ops, _, _ = _mods()
    table = R.pixel_tables(7, 32, 2, True, 0)
    for shape in ((7, 1, 1, 3), (7, 32, 32, 2), (7, 32, 32, 5)):
        pool = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        big, out = _guarded(2, shape[1], shape[3])
        with pytest.raises(lib.ObbHipError):
            ops.aug_tiles(pool, _dev_table(A, table), True, False, out=out)
        assert bool((big == 0xAB).all())
    # a source index outside the pool, or a centre outside the canvas: the entry cannot see the device table, the tile's workgroups write nothing;
    # the other tile of the same call is written.  The host-side check of the Python layer raises before anything is launched.
    s, pool = 32, R.random_pool(7, 32, 4, 1)
    for field, value in (("src", 7), ("src", -1), ("xc", 2 * s + 1)):
        bad = table.copy()
        if field == "src":
            bad["src"][1, 2] = value
        else:
            bad[field][1] = value
        big, out = _guarded(2, s, 4)
        ops.aug_tiles(torch.from_numpy(pool).cuda(), _dev_table(A, bad), True, False, out=out)
        assert np.array_equal(out[0].cpu().numpy(), R.tiles_ref(pool, table[:1])[0])
        assert bool((big[2] == 0xAB).all()) and bool((big[0] == 0xAB).all()) and bool((big[3] == 0xAB).all())
        lab = torch.zeros((7, 2, 9), dtype=torch.float64, device="cuda")
        outs = (torch.full((2, 3), 77, dtype=torch.int32, device="cuda"), torch.full((2, 3, 5), 7.0, device="cuda"),
                torch.ones((2, 3), dtype=torch.bool, device="cuda"), torch.full((2,), 77, dtype=torch.int32, device="cuda"))
        ops.aug_labels(lab, torch.zeros(7, dtype=torch.int32, device="cuda"), _dev_table(A, bad), s, 3, out=outs)
        assert int(outs[3][0]) == 0 and int(outs[3][1]) == 77 and bool((outs[0][1] == 77).all()) and bool((outs[1][1] == 7.0).all()) and not bool(outs[2][0].any())
        with pytest.raises(ValueError):
            A.check_table(bad, 7, s)
    with pytest.raises(lib.ObbHipError):
        ops.aug_labels(torch.zeros((7, 2, 9), dtype=torch.float64, device="cuda"), torch.zeros(7, dtype=torch.int32, device="cuda"), _dev_table(A, table), 1, 3)


# ---------------------------------------------------------------- labels
def _run_labels(A, ops, s, lab, cnt, table, n_cap, guard=True):
    B = len(table)
    gl = torch.full((B + 2, n_cap), 77, dtype=torch.int32, device="cuda")
    gb = torch.full((B + 2, n_cap, 5), 7.0, dtype=torch.float32, device="cuda")
    mk = torch.ones((B + 2, n_cap), dtype=torch.bool, device="cuda")
    ct = torch.full((B + 2,), 77, dtype=torch.int32, device="cuda")
    ops.aug_labels(torch.from_numpy(lab).cuda(), torch.from_numpy(cnt).cuda(), _dev_table(A, table), s, n_cap, out=(gl[1:B + 1], gb[1:B + 1], mk[1:B + 1], ct[1:B + 1]))
    for t, v in ((gl, 77), (gb, 7.0), (ct, 77)):  # nothing outside the caller's buffers is touched
        assert bool((t[0] == v).all()) and bool((t[-1] == v).all())
    assert bool(mk[0].all()) and bool(mk[-1].all())
    return gl[1:B + 1].cpu().numpy(), gb[1:B + 1].cpu().numpy(), mk[1:B + 1].cpu().numpy(), ct[1:B + 1].cpu().numpy()


def _check_labels(got, exp, s, name):
    gl, gb, mk, ct = got
    el, eb, em, ec = exp[:4]
    assert np.array_equal(ct, ec), (name, ct, ec)
    assert np.array_equal(mk, em) and np.array_equal(gl, el), name
    err, tol = np.abs(gb.astype(np.float64) - eb), box_tol(eb, s)
    print(f"{name}: survivors {ec.tolist()}, max |box - ref| / tol = {float((err / tol).max()) if err.size else 0.0:.3f}")
    assert (err <= tol).all(), (name, np.argwhere(err > tol)[:4].tolist(), float((err / tol).max()))
    assert not gb[~mk].any() and not gl[~mk].any()  # rows behind the survivors are zero


@pytest.mark.parametrize("case", R.label_cases(), ids=lambda c: c[0])
def test_labels_against_reference(case):
    _, A, ops, _, _ = _mods()
    name, s, lab, cnt, table, n_cap = case
    exp = R.labels_ref(lab, cnt, table, s, n_cap)
    got = _run_labels(A, ops, s, lab, cnt, table, n_cap)
    _check_labels(got, exp, s, name)
    again = _run_labels(A, ops, s, lab, cnt, table, n_cap)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))  # bit-identical on repeat
    if name == "pentagon":
        assert exp[3][0] == 2 and len(R.clip_square(R.hull([tuple(p) for p in _warped(table[0], lab[0, 0], s)]), s)) == 5
    if name == "clipped-away":
        assert exp[3][0] == 1 and exp[0][0, 0] == 2
    if name == "n_cap-2":
        assert (exp[3] > n_cap).any() and len(exp[4]) == exp[3].sum()  # count is exact past n_cap; the rows kept are the reference's first rows
    if name == "empty-pool":
        assert not exp[3].any()


def _warped(rec, row, s):
    M = rec["fwd"]
    return [((M[0] * x + M[1] * y) + M[2], (M[3] * x + M[4] * y) + M[5]) for x, y in (np.asarray(row[1:]).reshape(4, 2) * s)]


def test_labels_square_is_a_tie():
    """A square: both edge directions give the same rectangle and (w, h, theta) may legitimately come out as (h, w, theta +- pi/2), which the loss and
    the assigner cannot tell apart.  Compared through the centre and the ProbIoU covariance (a, b, c) = (w^2 cos^2 + h^2 sin^2, w^2 sin^2 + h^2 cos^2,
    (w^2 - h^2) cos sin) / 12.  Bound: w and h carry 2^-24 relative (fp32), their squares 2^-23; theta carries 2^-24 * pi/2 and d(a, b, c)/d theta is at
    most |w^2 - h^2| / 12 <= a + b: in all under 4 * 2^-23 (a + b), plus the fp64 term on a quantity of size s^2."""
    _, A, ops, _, _ = _mods()
    s = 64
    lab, cnt = np.zeros((1, 1, 9)), np.array([1], np.int32)
    lab[0, 0] = R.rect_row(4, 30, 34, 20, 20, 0.4, s)
    table = np.zeros(1, A.REC)
    A.make_record(table[0], A.affine(s, s, 17.0, 1.1, 0.52, 0.47), 1.1, s, fliplr=True)
    exp = R.labels_ref(lab, cnt, table, s, 2)
    gl, gb, mk, ct = _run_labels(A, ops, s, lab, cnt, table, 2)
    assert ct[0] == 1 == exp[3][0] and gl[0, 0] == 4 and mk[0].tolist() == [True, False]
    g, e = gb[0, 0].astype(np.float64), exp[1][0, 0]
    assert (np.abs(g[:2] - e[:2]) <= box_tol(e[:2], s)).all()
    assert 0.0 <= g[4] <= np.float32(math.pi / 2)

    def cov(b):
        w2, h2, c, sn = b[2] ** 2 / 12, b[3] ** 2 / 12, math.cos(b[4]), math.sin(b[4])
        return np.array([w2 * c * c + h2 * sn * sn, w2 * sn * sn + h2 * c * c, (w2 - h2) * c * sn])
    cg, ce = cov(g), cov(e)
    tol = 4 * 2.0 ** -23 * (ce[0] + ce[1]) + 1e-12 * s * s
    print("square: device", g.tolist(), "reference", list(e), "max |d cov| / tol", float(np.abs(cg - ce).max() / tol))
    assert (np.abs(cg - ce) <= tol).all()
    assert abs(e[2] - 22.0) < 1e-9 and abs(e[3] - 22.0) < 1e-9  # 20 px at scale 1.1


# ---------------------------------------------------------------- capture
def test_batch_into_replays_under_graph_capture():
    _, A, ops, _, _ = _mods()
    s, N, B = 40, 7, 3
    pool = R.random_pool(N, s, 3, seed=21)
    lab, cnt = R.label_pool(N, 5, s, seed=22, empty=(2,))
    bt = A.TrainBatcher(torch.from_numpy(pool).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(cnt).cuda(), A.AugmentConfig(), n_cap=12)
    p1 = A.sample_params(bt.cfg, B, N, s, np.random.RandomState(1), [0, 3, 6])
    p2 = A.sample_params(bt.cfg, B, N, s, np.random.RandomState(2), [5, 2, 1])
    eager = []
    for p in (p1, p2):
        out = bt.batch(None, None, params=p)
        eager.append([t.clone() for t in out] + [bt.count.clone()])
    bufs = bt.buffers(B)
    bt.write_table(bufs[0], p1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bt.batch_into(*bufs)
    for p, exp in ((p1, eager[0]), (p2, eager[1])):
        bt.write_table(bufs[0], p)  # in place: the captured kernels read the same address
        for t in bufs[1:]:
            t.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        for got, e in zip(bufs[1:], exp):
            assert torch.equal(got, e)
    assert not torch.equal(eager[0][0], eager[1][0])
    # and the eager batches are the reference's (RGB out of a BGR pool)
    assert np.array_equal(eager[1][0].cpu().numpy(), R.tiles_ref(pool, p2, True, True))


# ---------------------------------------------------------------- into the net
def test_batch_from_the_tiler_into_the_net():
    _, A, ops, tiler, TR = _mods()
    import net_ref as NR
    s, B = 64, 2
    rng = np.random.RandomState(8)
    img = rng.randint(0, 256, (160, 208, 3)).astype(np.uint8)
    labels = np.array([np.concatenate([[c], R.xywhr_corners(b).reshape(8)]) for c, b in
                       [(3, (50, 40, 30, 18, 0.3)), (1, (120, 60, 26, 40, -0.5)), (7, (90, 110, 34, 22, 1.0)), (5, (170, 100, 28, 28, 0.2)), (2, (30, 120, 20, 30, 0.7))]])
    positives, empties = tiler.tile_image(img, labels, tile_size=s, overlap=16)
    assert len(positives) >= 3
    dimg = torch.from_numpy(img).cuda()
    crops = [dimg[e["y"]:e["y"] + s, e["x"]:e["x"] + s].contiguous() for e in tiler.select_empty_tiles(empties, 1.0)]
    bt = A.TrainBatcher.from_tiler(positives, crops, A.AugmentConfig(), n_cap=8)
    N = bt.N
    assert N == len(positives) + len(crops) and bt.labels.shape[0] == N
    params = A.sample_params(bt.cfg, B, N, s, np.random.RandomState(4), [0, 1])
    lab, cnt = bt.labels.cpu().numpy(), bt.counts.cpu().numpy()
    exp = R.labels_ref(lab, cnt, params, s, 64)
    rows = [(b, c, x / s, y / s, w / s, h / s, t) for b, c, x, y, w, h, t in exp[4]]
    assert len(rows) >= 2
    pl, pb, pm = TR.pad_targets(rows, B, s)
    bt.n_cap = pl.shape[1]  # n_cap = pad_targets' n_max
    tiles, gl, gb, mk = bt.batch([0, 1], None, params=params)
    assert np.array_equal(tiles.cpu().numpy(), R.tiles_ref(bt.tiles.cpu().numpy(), params, True, True))
    assert torch.equal(gl.cpu(), pl) and torch.equal(mk.cpu(), pm)
    eb = R.labels_ref(lab, cnt, params, s, bt.n_cap)[1]
    assert (np.abs(gb.cpu().numpy().astype(np.float64) - eb) <= box_tol(eb, s)).all()
    assert np.array_equal(bt.count.cpu().numpy(), exp[3])
    net = TR.Net.from_state({k: v.cuda() for k, v in NR.make_state("n", 12, 3, seed=5).items()}, "n", 12, 3)
    items = net.forward_backward(tiles, gl, gb, mk)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(items).all()) and float(items.sum()) > 0
