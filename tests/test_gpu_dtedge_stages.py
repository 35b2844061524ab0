"""The 4-channel input builder (csrc/dtedge.hip) stage by stage against oracle/dtedge.py, over the case table of tests/dtedge_cases.py (every
branch of the radix select: see tests/test_dtedge_cases_cpu.py), over the launcher's documented domain, and over many crops per call.

Every comparison is exact -- the kernels restate the oracle operation for operation: acc and dist as uint32 bit patterns (distances beyond
the 99th percentile included, which the final byte clips), thr / lo / hi as float64 bit patterns of numpy's percentile, mn / mx as float32.
A mismatch names the FIRST stage of the pipeline that differs, with the pixel."""
import ctypes as C

import numpy as np
import pytest
import torch

import dtedge_cases as dc
from oracle import dtedge as od

pytestmark = pytest.mark.gpu


def _ops():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    return ops


def _run(batch):
    """uint8 [B,h,w,3] -> numpy (out, acc, edges, dist, stats) of one call"""
    return tuple(t.cpu().numpy() for t in _ops().build_multich_stages(torch.as_tensor(np.ascontiguousarray(batch)).cuda()))


def _image_diff(name, got, exp):
    if got.dtype == np.float32:
        got, exp = got.view(np.uint32), np.ascontiguousarray(exp, np.float32).view(np.uint32)
    bad = got != exp
    if not bad.any():
        return None
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    return "%s differs at %d pixel(s), first at (y, x%s) = %s: device %r, oracle %r" % (
        name, int(bad.sum()), ", c" if got.ndim == 3 else "", idx, got[idx], exp[idx])


def _scalar_diff(name, got, exp, f32):
    g, e = (np.float32(got).view(np.uint32), np.float32(exp).view(np.uint32)) if f32 else (np.float64(got).view(np.uint64), np.float64(exp).view(np.uint64))
    if g == e and (not f32 or float(np.float32(got)) == float(got)):
        return None
    return "%s differs: device %r (%#x), oracle %r (%#x)" % (name, float(got), int(g), float(exp), int(e))


def first_difference(got, k, exp):
    """None, or what the first differing stage of crop k is -- in the order in which the six launches produce them"""
    out, acc, edges, dist, stats = (g[k] for g in got)
    e_acc, e_edges, e_dist, (thr, lo, hi, mn, mx), e_out = exp
    checks = (lambda: _image_diff("acc", acc, e_acc),
              lambda: _scalar_diff("thr (90th percentile of acc)", stats[0], thr, False),
              lambda: _scalar_diff("mn (min of acc)", stats[3], mn, True),
              lambda: _scalar_diff("mx (max of acc)", stats[4], mx, True),
              lambda: _image_diff("edges", edges, e_edges),
              lambda: _image_diff("dist", dist, e_dist),
              lambda: _scalar_diff("lo (1st percentile of dist)", stats[1], lo, False),
              lambda: _scalar_diff("hi (99th percentile of dist)", stats[2], hi, False),
              lambda: _image_diff("out", out, e_out))
    for c in checks:
        msg = c()
        if msg:
            return msg
    return None


def _assert_equal(batch, exps=None, what=""):
    got = _run(batch)
    assert got[0].shape == batch.shape[:3] + (4,) and got[4].shape == (len(batch), 5)
    for k in range(len(batch)):
        exp = exps[k] if exps is not None else od.stages(batch[k])
        msg = first_difference(got, k, exp)
        assert msg is None, "%s crop %d of %d, %d x %d: %s" % (what, k, len(batch), batch.shape[1], batch.shape[2], msg)
    return got


# ------------------------------------------------------------------------------------------------ 1. every case of the table

@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_stages_equal_the_oracle_on_the_case_table(case):
    img = dc.make(case)
    got = _assert_equal(img[None], [dc.oracle_stages(case)], dc.case_id(case))
    assert np.array_equal(got[0], _ops().build_multich(torch.as_tensor(img[None]).cuda()).cpu().numpy())  # the plain entry point: same bytes


# ------------------------------------------------------------------------------------------------ 2. the documented domain

SWEEP = [(15, 16), (16, 15), (16, 16), (16, 300), (300, 16), (2, 1024), (4096, 2),                              # the SMALL switch of k_dt_acc
         (20, 127), (20, 128), (20, 255), (20, 256), (20, 511), (20, 512), (20, 1023), (20, 1024),             # lane-class edges (w == pitch)
         (31, 63), (32, 64), (33, 65),                                                                          # tile edges
         (4096, 18), (2049, 130),                                                                               # row ring, overshoot row, large n
         (600, 1024)]


@pytest.mark.parametrize("h,w", SWEEP, ids=lambda v: str(v))
def test_domain_sweep(h, w):
    crops = [dc.strokes(h, w, 1000 + h * 7 + w)]
    if h * w <= 100000:
        crops.append(dc.strokes(h, w, 2000 + h * 7 + w)[::-1, ::-1].copy())
    _assert_equal(np.stack(crops), what="sweep")


@pytest.mark.parametrize("h", range(2, 8))
def test_fewer_rows_than_the_chamfer_ring(h):
    """h < the depth-4 row ring, and every h % 4"""
    _assert_equal(np.stack([dc.strokes(h, 70, 50 + h), dc.noise(h, 70, 60 + h)]), what="short")


# ------------------------------------------------------------------------------------------------ 3. batch and workspace

def _mixed(h, w, k):
    """distinct content per k: different statistics (thr, lo, hi, mn, mx all differ from crop to crop)"""
    kind = (dc.strokes, dc.noise, dc.blobs)[k % 3]
    img = kind(h, w, 300 + k)
    return img if k % 2 == 0 else (img // (1 + k % 5) + 3 * k).astype(np.uint8)


def test_many_distinct_crops_in_one_call():
    batch = np.stack([_mixed(45, 130, k) for k in range(37)])
    got = _assert_equal(batch, what="B = 37")
    assert len({got[4][k].tobytes() for k in range(37)}) >= 30                      # the per-crop statistics really differ


def test_workspace_growth_and_reuse_between_calls():
    """small, large (the workspace grows), small again on one context and stream; the large call's 37 crops are drawn from 5 distinct images
    (their order has no period), each compared with its own oracle"""
    small = np.stack([dc.strokes(16, 16, 5)])
    small2 = np.stack([dc.strokes(16, 16, 5), dc.noise(16, 16, 6)])
    distinct = [_mixed(200, 520, k) for k in range(5)]
    exps = [od.stages(im) for im in distinct]
    order = [(k * k + k // 3) % 5 for k in range(37)]
    first = _assert_equal(small, what="before")
    _assert_equal(np.stack([distinct[i] for i in order]), [exps[i] for i in order], what="large")
    again = _assert_equal(small2, what="after")
    for a, b in zip(first, again):
        assert np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8))


def test_empty_batch():
    ops = _ops()
    empty = torch.empty((0, 8, 8, 3), dtype=torch.uint8, device="cuda")
    res = ops.build_multich_stages(empty)
    assert tuple(res[0].shape) == (0, 8, 8, 4) and tuple(res[1].shape) == (0, 8, 8) and tuple(res[4].shape) == (0, 5)
    assert tuple(ops.build_multich(empty).shape) == (0, 8, 8, 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. rejections

@pytest.mark.parametrize("h,w", [(1, 8), (8, 1), (8, 1025), (4097, 8)])
def test_read_out_rejects_what_build_multich_rejects(h, w):
    ops = _ops()
    x = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        ops.build_multich(x)
    with pytest.raises(RuntimeError):
        ops.build_multich_stages(x)
    torch.cuda.synchronize()


def test_null_buffers_are_refused():
    ops = _ops()
    from oriented_object_detection_amd import _lib
    L = _lib.lib()
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
    assert L.obb_build_multich_stages(ops.ctx(), None, 1, 8, 8, po, None, None, None, None, s) < 0
    assert L.obb_build_multich_stages(ops.ctx(), px, 1, 8, 8, None, None, None, None, None, s) < 0
    assert L.obb_build_multich(ops.ctx(), None, 1, 8, 8, po, s) < 0
    assert L.obb_build_multich(ops.ctx(), px, 1, 8, 8, None, s) < 0
    assert L.obb_build_multich_stages(ops.ctx(), px, 1, 8, 8, po, None, None, None, None, s) == 0   # every read-out pointer NULL: allowed
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], od.build_multich(np.zeros((8, 8, 3), np.uint8), 4))
