"""The one-launch weight pack (csrc/convgrad.hip k_pack_conv_multi_bf16; ops.conv_pack_plan / conv_pack_multi_bf16; train.PackPlan) against the
per-layer pack it replaces: every dense conv of YOLO11-OBB n and s at four tile sizes, both forms, bit for bit; nothing written outside the
segments; replay inside a captured graph; refusals write nothing; with a plan attached a Net never packs per layer."""
import ctypes as C

import pytest
import torch

import net_ref as NR
from bounds import Guarded

pytestmark = pytest.mark.gpu

SENT = 0x7FC1  # a bf16 NaN pattern no pack produces from finite weights


def _mods():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops, train
    return _lib, ops, train


def _flat_of(layers, seed):
    """-> (flat fp32 Guarded, [(w view, offset)]) with every layer's [cout,cin,k,k] weights back to back behind an odd-sized gap"""
    g = torch.Generator().manual_seed(seed)
    sizes = [co * ci * k * k for _, co, ci, k, _, _, _ in layers]
    gap = 24  # (the first layer does not start at element 0)
    G = Guarded((gap + sum(sizes),), torch.float32, torch.randn(gap + sum(sizes), generator=g))
    views, off = [], gap
    for (_, co, ci, k, _, _, _), n in zip(layers, sizes):
        views.append((G.out[off:off + n].view(co, ci, k, k), off))
        off += n
    return G, views


def _plan_layers(layers, views):
    recs = []
    for (_, co, ci, k, s, H, W), (_, off) in zip(layers, views):
        recs += [(co, ci, k, s, H, W, f, off) for f in (0, 1)]
    return recs


@pytest.mark.parametrize("scale", ["n", "s"])
@pytest.mark.parametrize("H,W", [(416, 416), (128, 128), (64, 64), (64, 96)])
def test_every_segment_equals_the_per_layer_pack(scale, H, W):
    _lib, ops, _ = _mods()
    layers = NR.dense_layers(scale, 12, 3, H, W)
    assert len(layers) >= 60 and any(s == 2 for *_, s, _, _ in layers) and any(n.endswith("cv2.0.2") for n, *_ in layers)
    F, views = _flat_of(layers, seed=H + W)
    plan = ops.conv_pack_plan("cuda", _plan_layers(layers, views), F.out.numel())
    assert plan.nrec == 2 * len(layers) and plan.total % 256 == 0 and all(d % 256 == 0 for d in plan.dst_off)
    assert plan.dst_off == sorted(plan.dst_off) and plan.dst_off[-1] + plan.n_elems[-1] <= plan.total
    P = Guarded((plan.total,), torch.bfloat16)
    P.out.view(torch.int16).fill_(SENT)
    ops.conv_pack_multi_bf16(F.out, plan, out=P.out)
    torch.cuda.synchronize()
    assert P.guards_intact() and F.guards_intact()
    covered = torch.zeros(plan.total, dtype=torch.bool, device="cuda")
    for i, ((name, co, ci, k, s, h, w), (wv, _)) in enumerate(zip(layers, views)):
        for f in (0, 1):
            d, n = plan.dst_off[2 * i + f], plan.n_elems[2 * i + f]
            ref = ops.conv_pack_bf16(wv, h, w, dgrad_form=bool(f), stride=s)
            assert ref.numel() == n, (name, f)
            assert torch.equal(P.out[d:d + n].view(torch.int16), ref.view(torch.int16)), (name, f, h, w)
            covered[d:d + n] = True
    pad = P.out.view(torch.int16)[~covered]
    assert bool((pad == SENT).all()), "padding between segments was written"


def test_replay_inside_a_graph_is_bit_identical():
    _lib, ops, _ = _mods()
    layers = NR.dense_layers("n", 12, 3, 64, 96)
    F, views = _flat_of(layers, seed=7)
    plan = ops.conv_pack_plan("cuda", _plan_layers(layers, views), F.out.numel())
    out = torch.zeros(plan.total, dtype=torch.bfloat16, device="cuda")
    ops.conv_pack_multi_bf16(F.out, plan, out=out)  # (warm-up outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.conv_pack_multi_bf16(F.out, plan, out=out)
    for seed in (11, 12):
        F.out.copy_(torch.randn(F.out.numel(), generator=torch.Generator().manual_seed(seed)))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = ops.conv_pack_multi_bf16(F.out, plan)
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
        (name, co, ci, k, s, h, w), (wv, _) = layers[5], views[5]
        assert torch.equal(out[plan.dst_off[10]:plan.dst_off[10] + plan.n_elems[10]].view(torch.int16), ops.conv_pack_bf16(wv, h, w, stride=s).view(torch.int16))


def test_refusals_write_nothing():
    _lib, ops, TR = _mods()
    L = _lib.lib()
    layers = NR.dense_layers("n", 12, 3, 64, 64)
    F, views = _flat_of(layers, seed=3)
    recs = _plan_layers(layers, views)
    plan = ops.conv_pack_plan("cuda", recs, F.out.numel())
    other = ops.conv_pack_plan("cuda", _plan_layers(NR.dense_layers("n", 12, 3, 416, 416), views), F.out.numel())
    assert other.total != plan.total and other.nrec == plan.nrec  # (13-multiple maps take another layout)
    P = Guarded((max(plan.total, other.total),), torch.bfloat16)
    P.out.view(torch.int16).fill_(SENT)
    ctx, st = ops.ctx("cuda"), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    tw, n = plan.table.numel(), plan.nrec
    calls = {
        "table too short": (p(F.out), F.out.numel(), p(plan.table), tw - 8, n, p(P.out), plan.total),
        "table too long": (p(F.out), F.out.numel(), p(plan.table), tw + 1, n, p(P.out), plan.total),
        "no records": (p(F.out), F.out.numel(), p(plan.table), tw, 0, p(P.out), plan.total),
        "total no multiple of 256": (p(F.out), F.out.numel(), p(plan.table), tw, n, p(P.out), plan.total - 8),
        "NULL weights": (C.c_void_p(0), F.out.numel(), p(plan.table), tw, n, p(P.out), plan.total),
        "NULL table": (p(F.out), F.out.numel(), C.c_void_p(0), tw, n, p(P.out), plan.total),
        "NULL output": (p(F.out), F.out.numel(), p(plan.table), tw, n, C.c_void_p(0), plan.total),
    }
    for what, a in calls.items():
        assert L.obb_conv_pack_multi_bf16(ctx, *a, st) == -1, what  # OBB_ERR_INVALID
    # a table planned for another map size, or a flat buffer shorter than the plan reads: launched, and every workgroup returns before its first store
    assert L.obb_conv_pack_multi_bf16(ctx, p(F.out), F.out.numel(), p(plan.table), tw, n, p(P.out), other.total, st) == 0
    assert L.obb_conv_pack_multi_bf16(ctx, p(F.out), F.out.numel(), p(other.table), tw, n, p(P.out), plan.total, st) == 0
    assert L.obb_conv_pack_multi_bf16(ctx, p(F.out), F.out.numel() - 64, p(plan.table), tw, n, p(P.out), plan.total, st) == 0
    torch.cuda.synchronize()
    assert P.guards_intact() and bool((P.out.view(torch.int16) == SENT).all()), "a refused call wrote"
    with pytest.raises(ValueError):
        ops.conv_pack_multi_bf16(F.out, other, out=P.out[:plan.total])
    with pytest.raises(ValueError):
        ops.conv_pack_multi_bf16(F.out[:-4], plan)
    # the plan entry: a record reading past the flat buffer, k = 1 at stride 2, NULL outputs -> refused, nothing returned
    with pytest.raises(_lib.ObbHipError):
        ops.conv_pack_plan("cuda", recs, F.out.numel() - 64)
    with pytest.raises(ValueError):
        ops.conv_pack_plan("cuda", [(16, 16, 1, 2, 8, 8, 0, 0)], 4096)
    with pytest.raises(_lib.ObbHipError):
        ops.conv_pack_plan("cuda", [(16, 16, 3, 1, 8, 8, 0, -1)], 4096)
    # and the good call still works afterwards
    ops.conv_pack_multi_bf16(F.out, plan, out=P.out[:plan.total])
    torch.cuda.synchronize()
    wv = views[0][0]
    _, co, ci, k, s, h, w = layers[0]
    assert torch.equal(P.out[:plan.n_elems[0]].view(torch.int16), ops.conv_pack_bf16(wv, h, w, stride=s).view(torch.int16))


def test_packplan_views_and_other_map_size():
    """train.PackPlan on a ConvBN pair: forward and backward through the views equal the per-call packing bit for bit; another H x W raises."""
    _lib, ops, TR = _mods()
    g = torch.Generator().manual_seed(9)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    outs = []
    for attach in (False, True):
        groups = TR.ParamGroups()
        g.manual_seed(9)
        a = TR.ConvBN(groups, mk(32, 16, 3, 3) * 0.1, s=2)
        b = TR.ConvBN(groups, mk(24, 32, 1, 1) * 0.2)
        groups.build()
        x = (torch.randn(2, 12, 20, 16, generator=torch.Generator().manual_seed(1)) * 1.0).to(torch.bfloat16).cuda()
        da = torch.randn(2, 6, 10, 24, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
        if attach:
            plan = TR.PackPlan(groups, [a, b], [(12, 20), (6, 10)])
            plan.run()
        y = b.forward(a.forward(x))
        dx = a.backward(b.backward(da))
        outs.append((y, dx, groups.opts[0].grad.clone()))
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    with pytest.raises(ValueError, match="planned for"):
        a.forward(torch.zeros(2, 16, 16, 16, dtype=torch.bfloat16, device="cuda"))
    plan.detach()
    assert a.pack is None and b.pack is None
    a.forward(torch.zeros(2, 16, 16, 16, dtype=torch.bfloat16, device="cuda"))  # per-call packing again


def test_net_with_a_plan_never_packs_per_layer(monkeypatch):
    _lib, ops, TR = _mods()
    st = {k: v.cuda() for k, v in NR.make_state("n", 12, 3, seed=4).items()}
    net = TR.Net.from_state(st, "n", 12, 3)
    tiles = torch.randint(0, 256, (2, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    gl, gb, mk = TR.pad_targets([[0, 3, 0.5, 0.5, 0.4, 0.3, 0.2], [1, 7, 0.4, 0.6, 0.5, 0.5, 1.0]], 2, (64, 64), device="cuda")
    calls = []
    real = ops.conv_pack_bf16
    monkeypatch.setattr(ops, "conv_pack_bf16", lambda *a, **k: (calls.append(a), real(*a, **k))[1])
    items = net.forward_backward(tiles, gl, gb, mk)
    torch.cuda.synchronize()
    assert not calls and bool(torch.isfinite(items).all())
    n_dense = sum(1 for _, b in net.named_blocks() if hasattr(b, "_packed"))
    assert net.plan.table.nrec == 2 * n_dense
    net2 = TR.Net.from_state(st, "n", 12, 3, pack=False)
    net2.forward_backward(tiles, gl, gb, mk)
    assert len(calls) == 2 * n_dense  # (the per-layer path: two packs per dense conv and iteration)
