"""The fp64 post-processing reference (postproc_ref.py) and its committed inputs, without a GPU:
  * it agrees with the fp32 torch oracle (oracle/postproc.py) on every committed case: same kept sets in the same order, decode within E;
  * every committed case is fully decided (cap on undecided pairs, candidates, classes and ties: zero);
  * every mutation of the reference changes the output of a committed case at every threshold.  `>` for `>=` needs a deviation: a
    decided case has no pair with iou == thr, so the reference and its `>` mutation both run on the committed case with the threshold
    moved (by less than 0.02) onto the exact fp64 IoU of one of its own pairs, the strongest suppressor of one row; the last-maximum
    mutation runs on the duplicate-maxima case;
  * the cases populate the branches they are meant for (printed with -s)."""
import pytest
import torch

import postproc_ref as R
from oracle import postproc as pp

MATRIX = [(nc, conf) for nc in R.NMS_NC for conf in R.NMS_CONF]


def _oracle_rows(head, h, w, nc, conf, thr, max_det):
    pred = pp.decode(head[..., :64 + nc + 1].contiguous(), h, w, nc)
    return pp.non_max_suppression(pred, conf, thr, max_det, nc)


def _agree(syn, cases, thresholds, max_dets):
    head = syn.tensor()
    ref, E = R.decode_bounds(head, syn.h, syn.w, syn.nc)
    got = pp.decode(head[..., :64 + syn.nc + 1].contiguous(), syn.h, syn.w, syn.nc).transpose(1, 2).double()
    ratio = ((got - ref).abs() / E).max()
    print(f"  decode: fp32 oracle worst |err| / E = {float(ratio):.3f}")
    assert ratio <= 1
    nc = syn.nc
    for thr in thresholds:
        for md in max_dets:
            exp = _oracle_rows(head, syn.h, syn.w, nc, syn.conf, thr, md)
            for b, c in enumerate(cases):
                rows, kept, _ = R.nms_run(c, thr, md)
                assert exp[b].shape[0] == len(kept), (thr, md, b, exp[b].shape, len(kept))
                if not len(kept):
                    continue
                a = c.anchor[kept]
                assert torch.equal(exp[b][:, 5].long(), c.cls[kept]), (thr, md, b)
                Eb = torch.cat([E[b, a, :4], E[b, a, 4:4 + nc].gather(1, c.cls[kept, None]), torch.zeros(len(a), 1), E[b, a, 4 + nc:]], 1)
                assert bool(((exp[b].double() - rows).abs() <= Eb).all()), (thr, md, b)


@pytest.mark.parametrize("nc,conf", MATRIX)
def test_matrix_case_is_decided_populated_and_agrees_with_the_fp32_oracle(nc, conf):
    syn, cases = R.nms_matrix_case(nc, conf)
    band = {t: 0 for t in R.THRESHOLDS}
    ties = 0
    for b, c in enumerate(cases):
        R.assert_decided(c, R.THRESHOLDS)
        assert c.n == R.NMS_TILES[b]
        ties += int((c.conf[:-1] == c.conf[1:]).sum()) if c.n > 1 else 0
        for t in R.THRESHOLDS:
            _, kept, nsupp = R.nms_run(c, t, 300)
            rep = R.pair_report(c, t)
            print(f"  nc {nc} conf {conf} image {b}: candidates {c.n} thr {t} suppressed {nsupp} kept {len(kept)} margin {rep['margin']:.1f} "
                  f"far {rep.get('far')} near {rep.get('near')} band {rep.get('band')}")
            assert rep["margin"] > R.MARGIN
            if c.n >= 256:
                assert nsupp >= 20
                if t > 1e-3:
                    assert rep["far"] > 0 and rep["near"] > 0
                    band[t] += rep["band"]
    assert ties >= 3, "tie blocks: equal confidences among the candidates"
    print(f"  nc {nc} conf {conf}: pairs inside the fast-decision guard band per threshold {band}")
    assert len(R.nms_run(cases[-1], 0.7, 300)[1]) > 40, "survivors must exceed max_det 40 and 5 in the largest image"
    _agree(syn, cases, R.THRESHOLDS, R.NMS_MAX_DET)


@pytest.mark.parametrize("conf", R.THIN_CONF)
@pytest.mark.parametrize("h,w", list(R.THIN_TILES))
def test_thin_case_is_decided_populated_and_agrees_with_the_fp32_oracle(h, w, conf):
    """the thin-tile cases (32 x 416, 416 x 32: 273 anchors; 32 x 32: 21): every row decided, none left out"""
    syn, cases = R.thin_case(h, w, conf)
    assert syn.A == max(R.THIN_TILES[h, w]) and len(cases) == len(R.THIN_TILES[h, w])
    for b, c in enumerate(cases):
        R.assert_decided(c, R.THRESHOLDS)
        assert c.n == R.THIN_TILES[h, w][b]
        for t in R.THRESHOLDS:
            _, kept, nsupp = R.nms_run(c, t, 300)
            rep = R.pair_report(c, t)
            print(f"  thin {h}x{w} conf {conf} image {b}: candidates {c.n} thr {t} suppressed {nsupp} kept {len(kept)} margin {rep['margin']:.1f}")
            assert rep["margin"] > R.MARGIN
            if c.n >= 256:  # populated: suppression happens at every threshold (4 .. 13 px boxes: few pairs reach IoU 0.9)
                assert nsupp >= (20 if t < 0.9 else 5)
    # the largest image has every anchor a candidate, and both suppressed and surviving rows at iou 0.7
    _, kept, nsupp = R.nms_run(cases[-1], 0.7, 300)
    assert cases[-1].n == syn.A and nsupp > 0 and len(kept) > (40 if syn.A > 21 else 5)
    _agree(syn, cases, R.THRESHOLDS, R.NMS_MAX_DET)


@pytest.mark.parametrize("which", ["416", "640"])
def test_large_cases_are_decided_and_agree_with_the_fp32_oracle(which):
    syn, cases, thr = R.big_case(which)
    for c in cases:
        R.assert_decided(c, thr)
        assert c.n > 256
        for t in thr:
            rep = R.pair_report(c, t)
            _, kept, nsupp = R.nms_run(c, t, 300)
            print(f"  {which}: candidates {c.n} thr {t} suppressed {nsupp} kept {len(kept)} margin {rep['margin']:.1f} far {rep['far']} near {rep['near']} band {rep['band']}")
            assert nsupp >= 20 and rep["far"] > 0 and rep["near"] > 0
    _agree(syn, cases, thr, (300,))


@pytest.mark.parametrize("thr", [t for t in R.THRESHOLDS if t > 1e-3])
def test_guard_band_of_the_fast_decision_is_populated(thr):
    """at least one same-class, not-far-apart pair per threshold lies inside the band around -log(1 + 1e-7 - (1 - thr)^2): the exact
    fall-back of the fast decision runs (at 5e-4 the kernels switch the fast decision off)"""
    n = 0
    for nc, conf in ((12, 0.25), (1, 0.6), (80, 0.001)):
        n += sum(R.pair_report(c, thr)["band"] for c in R.nms_matrix_case(nc, conf)[1] if c.n > 1)
    print(f"  iou {thr}: {n} pairs inside the guard band")
    assert n >= 1


def _out(c, thr, md, mut=None):
    rows, kept, _ = R.nms_run(c, thr, md, mut)
    return rows


def _differs(a, b):
    return a.shape != b.shape or not torch.equal(a, b)


@pytest.mark.parametrize("thr", R.THRESHOLDS)
@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_changes_a_committed_case(mut, thr):
    first = [(12, 0.25), (17, 0.6), (80, 0.001), (1, 0.25), (16, 0.25)]
    for nc, conf in first + [m for m in MATRIX if m not in first]:
        syn, cases = R.dup_max_case() if mut == "last_max" else R.nms_matrix_case(nc, conf)
        nc, conf = syn.nc, syn.conf
        for b, c in enumerate(cases):
            if c.n < 2:
                continue
            if mut in ("no_offset", "last_max", "tie_desc", "angle_half", "wh_swap", "stride_shift"):
                m = R.nms_prepare(torch.from_numpy(syn.head[b]), syn.h, syn.w, nc, conf, mut=mut, floors=False)
                if any(_differs(_out(c, thr, md), _out(m, thr, md)) for md in R.NMS_MAX_DET):
                    return
            elif mut == "gt":
                # the row whose strongest suppressor is nearest the threshold; the threshold moved onto that pair's exact IoU
                col = torch.full((c.n,), -1.0, dtype=torch.float64).scatter_reduce(0, c.J, c.iou, "amax")
                col[col <= 0] = -1.0  # (far pairs all share the clamped value 1 - sqrt(1 + eps): not a pair of its own)
                j = int((col - thr).abs().argmin())
                t2 = float(col[j])
                if abs(t2 - thr) < 0.02:
                    a, b_ = R.nms_run(c, t2, c.n, exact=True), R.nms_run(c, t2, c.n, "gt", exact=True)
                    if _differs(a[0], b_[0]):
                        assert len(b_[1]) == len(a[1]) + 1 and j in b_[1].tolist() and j not in a[1].tolist()
                        return
            else:
                if any(_differs(_out(c, thr, md), _out(c, thr, md, mut)) for md in R.NMS_MAX_DET):
                    return
    raise AssertionError(f"mutation {mut} changes no committed case at iou {thr}")


@pytest.mark.parametrize("nc", [1, 4, 12, 15, 16, 17, 80])
def test_decode_bound_holds_for_the_fp32_oracle(nc):
    """the host's fp32 evaluation of the same formulas is inside E on every decode input"""
    for h, w in ((64, 96), (128, 128), (416, 288)):
        head = R.decode_inputs(h, w, nc, seed=h + nc)
        ref, E = R.decode_bounds(head, h, w, nc)
        got = pp.decode(head[..., :64 + nc + 1].contiguous(), h, w, nc).transpose(1, 2).double()
        r = (got - ref).abs() / E
        print(f"  nc {nc} {h}x{w}: box {float(r[..., :4].max()):.3f} cls {float(r[..., 4:4 + nc].max()):.3f} theta {float(r[..., -1].max()):.3f}")
        assert float(r.max()) <= 1
        # a mutated decode is far outside it
        for mut in ("angle_half", "stride_shift"):
            bad = R.decode64(head.double(), h, w, nc, mut=mut)
            assert float(((bad - ref).abs() / E).max()) > 100


def test_results_reference_agrees_with_the_fp32_oracle():
    det = R.results_rows()
    xywhr, pts, Ex, Ep, dec = R.results64(det)
    obb, corners = pp.construct_result(det, (416, 416), (416, 416))
    assert int(dec.sum()) > 300 and int((~dec).sum()) == 2  # (the two rows on a boundary are flagged)
    assert bool(((obb[:, :5].double() - xywhr).abs() <= Ex)[dec].all())
    assert bool(((corners.reshape(-1, 8).double() - pts).abs() <= Ep)[dec].all())
