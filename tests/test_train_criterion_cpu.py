"""CPU checks behind test_gpu_train_criterion.py: the fused criterion's entry points exist; the fp64 restatement (criterion_ref.py) agrees with
oracle/postproc.decode, with oracle/loss.py's terms and with a hand-written chain rule; torch's own fp32 evaluation lies inside every bound (the
calibration) and planted mistakes leave it; pad_targets' known answers; and the committed end-to-end seeds have no discrete assigner flip between
fp32 and fp64."""
import math
import os

import pytest
import torch

import criterion_ref as CR
from oracle import loss as ol
from oracle import postproc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((128, 128), 2, 12), ((96, 160), 2, 15), ((96, 160), 1, 1)]


def _flat(seed, imgsz, B, nc, dtype="bf16"):
    box, cls, ang = CR.make_head(seed, imgsz, B, nc, dtype)
    return CR.cat_levels(box), CR.cat_levels(cls), CR.cat_levels(ang)[..., 0]


def test_entry_points_exist():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops, train
    hdr = open(os.path.join(ROOT, "include", "obbhip.h")).read()
    for name in ("obb_crit_decode", "obb_crit_loss"):
        assert name + "(" in hdr and name in _lib.SIGNATURES
    assert "v8OBBLoss.__call__" in hdr
    assert callable(ops.crit_decode) and callable(ops.crit_loss)
    assert hasattr(torch.ops.obbhip, "crit_decode") and hasattr(torch.ops.obbhip, "crit_loss")
    for name in ("OBBCriterion", "DetectHead", "pad_targets"):
        assert hasattr(train, name)


@pytest.mark.parametrize("imgsz", [(128, 128), (96, 160)])
def test_decode_equals_oracle_decode(imgsz):
    B, nc = 2, 5
    box, cls, ang = (t.double() for t in _flat(7, imgsz, B, nc, "fp32"))
    ps, pb, ap, st = CR.decode_px(box, cls, ang, imgsz)
    want = postproc.decode(torch.cat([box, cls, ang[..., None]], -1), imgsz[0], imgsz[1], nc)  # [B, 4 + nc + 1, A]
    got = torch.cat([pb[..., :4], ps, pb[..., 4:]], -1).transpose(1, 2)
    assert float((got - want).abs().max()) <= 1e-12 * max(imgsz)


def test_terms_equal_oracle_terms():
    g = torch.Generator().manual_seed(0)
    logits = torch.randn((50, 64), generator=g, dtype=torch.float64)
    ltrb = torch.rand((50, 4), generator=g, dtype=torch.float64) * 14.5
    w = torch.rand(50, generator=g, dtype=torch.float64)
    assert abs(float((CR.dfl_rows(logits, ltrb) * w).sum() / 3.0) - float(ol.dfl_loss(logits, ltrb, w, 3.0))) <= 1e-12
    far = torch.tensor([[-3.0, 20.0, 14.995, 0.0]], dtype=torch.float64)  # both ends of the clamp
    got = CR.dfl_rows(logits[:1], CR.target_ltrb(torch.tensor([[0.0, 0.0, 1.0, 1.0, 0.0]], dtype=torch.float64), torch.tensor([[0.5, 0.5]], dtype=torch.float64)))
    assert torch.isfinite(got).all()
    assert abs(float(CR.dfl_rows(logits[:1], far.clamp(0, CR.DFL_HI))) - float(ol.dfl_loss(logits[:1], far, None, 1.0))) <= 1e-6
    x, t = torch.randn((40, 7), generator=g, dtype=torch.float64), torch.rand((40, 7), generator=g, dtype=torch.float64)
    import torch.nn.functional as F
    assert float(F.binary_cross_entropy_with_logits(x, t, reduction="none").sum() / 2.0) == float(ol.bce_loss(x, t, 2.0))
    p = torch.tensor([[10.0, 12.0, 8.0, 3.0, 0.3]], dtype=torch.float64)
    q = torch.tensor([[11.0, 11.0, 6.0, 4.0, 0.5]], dtype=torch.float64)
    hd, _ = CR.probiou_mc(p, q)
    assert abs(float(hd) - float(1 - ol.probiou(p, q))) <= 1e-14


@pytest.mark.parametrize("imgsz", [(128, 128), (96, 160)])
def test_hand_chain_rule_equals_autograd(imgsz):
    B, nc = 2, 3
    box, cls, ang = (t.double() for t in _flat(3, imgsz, B, nc, "fp32"))
    anc, _ = CR.anchors(imgsz)
    g = torch.Generator().manual_seed(1)
    gp = torch.randn((B, anc.shape[0], 5), generator=g, dtype=torch.float64)
    bx, an = box.clone().requires_grad_(True), ang.clone().requires_grad_(True)
    pred, _ = CR.decode(bx, an, anc)
    db, da = torch.autograd.grad((pred * gp).sum(), (bx, an))
    hb, ha = CR.chain_rule(box, ang, gp, anc)
    assert float((hb - db).abs().max()) <= 1e-10 and float((ha - da).abs().max()) <= 1e-10


def _ratios(got, ref, bound, keys=("items", "tss", "d_box", "d_cls", "d_ang")):
    out = {}
    for k in keys:
        d = (got[k].double() - ref[k]).abs()
        out[k] = float(torch.where(d == 0, torch.zeros_like(d), d / bound[k]).max())
    return out


@pytest.fixture(scope="module")
def cases():
    """per test shape: the fp32-valued inputs with a hand-built assignment, the fp64 reference and its bounds (computed once)"""
    out = []
    for i, (imgsz, B, nc) in enumerate(SHAPES):
        box, cls, ang = _flat(10 + i, imgsz, B, nc)
        tb, ts, fg = CR.hand_targets(10 + i, imgsz, B, nc, small_tss=(i == 2))
        ref, bound = CR.crit_bounds(box, cls, ang, tb, ts, fg, imgsz)
        out.append((imgsz, B, nc, box, cls, ang, tb, ts, fg, ref, bound))
    return out


def test_fp32_evaluation_lies_inside_every_bound(cases):
    for (imgsz, B, nc, box, cls, ang, tb, ts, fg, ref, bound) in cases:
        got = CR.crit_eval(box.float(), cls.float(), ang.float(), tb.float(), ts.float(), fg, imgsz)
        r = _ratios(got, ref, bound)
        print(f"calibration {imgsz} B={B} nc={nc}: torch fp32 worst |err| / bound", {k: round(v, 3) for k, v in r.items()})
        assert max(r.values()) <= 1, r


MISTAKES = ["swap_lt", "no_offset", "no_pi", "no_B", "wrong_gain", "no_clamp", "no_stride_div", "rev_levels"]


@pytest.mark.parametrize("variant", MISTAKES)
def test_planted_mistake_leaves_the_bound(cases, variant):
    for (imgsz, B, nc, box, cls, ang, tb, ts, fg, ref, bound) in cases:
        if variant == "rev_levels":  # the logits of the levels concatenated in the wrong order
            lv = lambda t: CR.cat_levels(CR.split_levels(t, imgsz), "rev_levels")
            got = CR.crit_eval(box.double(), lv(cls).double(), ang.double(), tb.double(), ts.double(), fg, imgsz)
        elif variant == "no_pi":  # pi dropped from d theta / d a: the angle gradient of the reference, over pi
            got = {k: v.clone() for k, v in ref.items()}
            got["d_ang"] = got["d_ang"] / math.pi
        elif variant == "no_B" and B == 1:
            continue  # (the factor is 1)
        else:
            got = CR.crit_eval(box.double(), cls.double(), ang.double(), tb.double(), ts.double(), fg, imgsz, variant=variant)
        assert max(_ratios(got, ref, bound).values()) > 1, f"{variant} at {imgsz} B={B} nc={nc} stays inside the bounds"


def test_planted_no_max_and_swapped_hw(cases):
    imgsz, B, nc, box, cls, ang, tb, ts, fg, ref, bound = cases[2]  # sum target_scores < 1 here
    assert float(ts.sum()) < 1 and float(ref["tss"]) == 1.0
    got = CR.crit_eval(box.double(), cls.double(), ang.double(), tb.double(), ts.double(), fg, imgsz, variant="no_max")
    assert max(_ratios(got, ref, bound).values()) > 1
    for c in cases[1:]:  # the non-square shape: each map walked column-major
        imgsz, B, nc, box, cls, ang, tb, ts, fg, ref, bound = c
        sw = lambda t: CR.cat_levels(CR.split_levels(t, imgsz), "swap_hw")
        got = CR.crit_eval(sw(box).double(), cls.double(), ang.double(), tb.double(), ts.double(), fg, imgsz)
        assert max(_ratios(got, ref, bound).values()) > 1


def test_pad_targets_known_answers():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import train
    rows = [(0, 3, 0.5, 0.25, 0.25, 0.5, 0.1),
            (2, 1, 0.1, 0.2, 0.5, 0.5, -0.2),
            (0, 7, 0.5, 0.5, 0.01, 0.5, 0.0),     # 1.6 px wide at W = 160: dropped
            (2, 0, 0.9, 0.9, 0.0125, 0.5, 0.3),   # exactly 2 px wide: kept
            (0, 5, 0.75, 0.75, 0.125, 0.0625, 1.0)]
    gl, gb, mk = train.pad_targets(rows, 3, (96, 160))
    assert gl.dtype == torch.int32 and gb.dtype == torch.float32 and mk.dtype == torch.bool
    assert gl.tolist() == [[3, 5], [0, 0], [1, 0]]
    assert mk.tolist() == [[True, True], [False, False], [True, True]]
    want = torch.tensor([[[80, 24, 40, 48, 0.1], [120, 72, 20, 6, 1.0]], [[0, 0, 0, 0, 0]] * 2, [[16, 19.2, 80, 48, -0.2], [144, 86.4, 2, 48, 0.3]]])
    assert torch.allclose(gb, want, rtol=1e-6, atol=0)
    gl, gb, mk = train.pad_targets([], 2, 128)
    assert tuple(gl.shape) == (2, 1) and tuple(gb.shape) == (2, 1, 5) and not mk.any()
    with pytest.raises(ValueError):
        train.pad_targets([(3, 0, 0.5, 0.5, 0.5, 0.5, 0.0)], 2, 128)


def assigner_inputs(case):
    imgsz, B, nc, dtype, seed = case
    box, cls, ang = _flat(seed, imgsz, B, nc, dtype)
    gl, gb, mk = CR.make_gt(seed, imgsz, B, nc)
    return box, cls, ang, gl, gb, mk


@pytest.mark.parametrize("case", CR.E2E_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-B{c[1]}-nc{c[2]}-{c[3]}-s{c[4]}")
def test_seeds_have_no_discrete_flip(case):
    """fp32 and fp64 evaluations of the oracle assigner on the fp64 / fp32 decode agree on every discrete output: nothing to exclude on the GPU"""
    imgsz = case[0]
    box, cls, ang, gl, gb, mk = assigner_inputs(case)
    outs = []
    for dt in (torch.float64, torch.float32):
        ps, pb, ap, _ = CR.decode_px(box.to(dt), cls.to(dt), ang.to(dt), imgsz)
        tl, tbx, tsc, fg, ti, _, _ = ol.rotated_tal_assign(ps, pb, ap, gl.long()[..., None], gb.to(dt), mk[..., None].to(dt))
        outs.append((tl, fg, ti, tbx.double(), tsc > 0))
    assert int(outs[0][1].sum()) >= 8  # (a case without foreground would be vacuous)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
