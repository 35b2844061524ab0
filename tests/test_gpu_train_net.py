"""train.Trunk / train.Net on the device, tolerance-free: the wiring of the whole graph read from `taps` (every module's input is what the yaml graph
builds from the tapped outputs; every fan-out gradient is bf16(fp32 + fp32) of its two tapped contributions in the documented order), the pack plan
against per-layer packing, Net against its parts driven by hand, and two trainer steps against the same iterations driven by hand.  The modules
of the trunk are then run by the fp64 references from their own tapped input and gradient (net_ref.module_refs) under block_ref's bound, and the
whole trunk is held against one plain fp64 autograd graph (figures only)."""
import pytest
import torch

import net_ref as NR

pytestmark = pytest.mark.gpu

ROWS = [[0, 3, 0.5, 0.5, 0.4, 0.3, 0.2], [0, 1, 0.3, 0.7, 0.3, 0.5, -0.4], [1, 7, 0.4, 0.6, 0.5, 0.5, 1.0]]


def _train():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import train
    return train


def _state(scale, ch, seed):
    return {k: v.cuda() for k, v in NR.make_state(scale, 12, ch, seed=seed).items()}


def _tiles(H, W, ch, seed=1, B=2):
    return torch.randint(0, 256, (B, H, W, ch), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).cuda()


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b)


def _state_of(net):
    """every flat buffer a step can change: parameters, gradients, running statistics"""
    return [o.param for o in net.groups.opts] + [o.grad for o in net.groups.opts] + [net.groups.buffers]


def _check_wiring(taps, head=True):
    NR.check_wiring(taps)


@pytest.mark.parametrize("H,W,ch", [(64, 64, 3), (64, 96, 3), (64, 64, 4)], ids=["64x64", "64x96", "64x64-ch4"])
def test_net_wiring_bit_for_bit(H, W, ch):
    TR = _train()
    net = TR.Net.from_state(_state("n", ch, seed=H + W + ch), "n", 12, ch)
    net.record_taps = True
    gt = TR.pad_targets(ROWS, 2, (H, W), device="cuda")
    items = net.forward_backward(_tiles(H, W, ch), *gt)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(items).all()) and float(items.sum()) > 0
    assert [tuple(t.shape[1:3]) for t in net.taps[23]["in"]] == [(H // 8, W // 8), (H // 16, W // 16), (H // 32, W // 32)]
    _check_wiring(net.taps, head=True)
    for o in net.groups.opts:
        assert bool(torch.isfinite(o.grad).all()) and float(o.grad.abs().max()) > 0
    # every layer received a gradient of its own: no dW is left at zero.  (The box and angle branches of a level are reached only through that
    # level's foreground anchors, and a 2 x 2 P5 map may have none: those two families are asked for at some level, the rest everywhere.)
    some = {"cv2": False, "cv4": False}
    for name, b in net.named_blocks():
        nz = float(b.dw.abs().max()) > 0
        fam = name.split(".")[2] if name.startswith("model.23.") else None
        if fam in some:
            some[fam] |= nz
        else:
            assert nz, name
    assert all(some.values()), some
    net.record_taps = False
    net.forward_backward(_tiles(H, W, ch), *gt)
    assert net.taps is None  # (filled only when asked)


def test_trunk_s_wiring_bit_for_bit():
    TR = _train()
    st = _state("s", 3, seed=21)
    groups = TR.ParamGroups()
    trunk = TR.Trunk(groups, st, "s")
    groups.build()
    trunk.record_taps = True
    feats = trunk.forward(_tiles(64, 64, 3))
    assert [tuple(f.shape) for f in feats] == [(2, 8, 8, 128), (2, 4, 4, 256), (2, 2, 2, 512)]
    g = torch.Generator().manual_seed(5)
    d = [(torch.randn(f.shape, generator=g) * 0.05).to(torch.bfloat16).cuda() for f in feats]
    trunk.backward(d)
    torch.cuda.synchronize()
    taps = trunk.taps
    taps[23] = {"in": feats, "din": d}  # (the three gradients stand in for the head's)
    _check_wiring(taps, head=True)
    assert bool(torch.isfinite(groups.opts[0].grad).all())
    for name, b in trunk.named_blocks():
        assert float(b.dw.abs().max()) > 0, name


def test_plan_equals_per_layer_packing_and_parts_by_hand():
    """Net with the pack plan == Net packing per layer == Trunk + DetectHead.forward_backward driven by hand, in every output and gradient bit."""
    TR = _train()
    st = _state("n", 3, seed=31)
    tiles, gt = _tiles(64, 96, 3, seed=2), TR.pad_targets(ROWS, 2, (64, 96), device="cuda")
    a, b, c = TR.Net.from_state(st, "n", 12, 3), TR.Net.from_state(st, "n", 12, 3, pack=False), TR.Net.from_state(st, "n", 12, 3, pack=False)
    a.record_taps = b.record_taps = True
    ia, ib = a.forward_backward(tiles, *gt), b.forward_backward(tiles, *gt)
    feats = c.trunk.forward(tiles)
    ic, dfe = c.head.forward_backward(feats, *gt)
    c.trunk.backward(dfe)
    torch.cuda.synchronize()
    assert a.plan is not None and b.plan is None
    assert _bits(ia, ib) and _bits(ia, ic)
    for x, y, z in zip(_state_of(a), _state_of(b), _state_of(c)):
        assert _bits(x, y) and _bits(x, z)
    for i in NR.ORDER:
        assert _bits(a.taps[i]["out"], b.taps[i]["out"]), i
    for u, v in zip(a.taps[23]["out"], b.taps[23]["out"]):
        assert all(_bits(p, q) for p, q in zip(u, v))
    # a second iteration at another tile size rebuilds the plan; the old layout is not read
    t2, g2 = _tiles(64, 64, 3, seed=3), TR.pad_targets(ROWS, 2, (64, 64), device="cuda")
    assert _bits(a.forward_backward(t2, *g2), b.forward_backward(t2, *g2))
    for x, y in zip(_state_of(a), _state_of(b)):
        assert _bits(x, y)


def test_two_steps_equal_the_iterations_by_hand():
    TR = _train()
    st = _state("n", 3, seed=41)
    gt = TR.pad_targets(ROWS, 2, (64, 64), device="cuda")
    sched = TR.Schedule(epochs=3, nb=10, lr0=0.003, lrf=0.05, batch=16, nbs=16)
    net, twin = TR.Net.from_state(st, "n", 12, 3), TR.Net.from_state(st, "n", 12, 3, pack=False)
    ema, ema2 = TR.ModelEMA(net.groups), TR.ModelEMA(twin.groups)
    net.update = TR.TrainerUpdate(net.groups, sched, ema=ema)
    fold0 = {k: (w.clone(), b.clone()) for k, (w, b) in net.fold().items()}
    for it, ni in enumerate((50, 51)):
        tiles = _tiles(64, 64, 3, seed=10 + it)
        items = net.step(tiles, *gt, ni=ni, epoch=0)
        items2 = twin.forward_backward(tiles, *gt)
        s = sched.at(ni, 0)
        assert s["accumulate"] == 1 and s["lr"][0] > 0
        clip = TR.clip_grad_norm(twin.groups, 10.0)
        twin.groups.step(s["lr"], s["momentum"], clip)
        ema2.update()
        torch.cuda.synchronize()
        assert _bits(items, items2) and _bits(net.last_clip, clip)
        for x, y in zip(_state_of(net) + ema.ema, _state_of(twin) + ema2.ema):
            assert _bits(x, y), (it, ni)
    fold = net.fold()
    assert set(fold) == set(NR.conv_table("n", 12, 3))
    moved = 0
    for name, blk in net.named_blocks():
        w, b = fold[name]
        if isinstance(blk, TR._BNBlock):
            f = blk.gamma / torch.sqrt(blk.running_var + blk.eps)
            we, be = blk.w * f.view(-1, 1, 1, 1), blk.beta - blk.running_mean * f
            if name.endswith("attn.qkv"):
                inv = torch.argsort(TR.qkv_device_order(blk.c1 // 64)).cuda()
                we, be = we[inv], be[inv]
        else:
            we, be = blk.w, blk.b
        assert torch.equal(w, we) and torch.equal(b, be), name
        moved += int(not torch.equal(w, fold0[name][0]))
    assert moved == len(fold)  # every layer's folded weights moved with the two steps


def _run_case(TR, scale, ch, H, W, seed):
    """-> (state dict on the CPU, tiles, trunk, taps) after one forward + backward with taps: the whole Net for n, the trunk under seeded
    gradients for s"""
    st = NR.make_state(scale, 12, ch, seed=seed)
    dev = {k: v.cuda() for k, v in st.items()}
    tiles = torch.randint(0, 256, (2, H, W, ch), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    if scale == "n":
        net = TR.Net.from_state(dev, "n", 12, ch)
        net.record_taps = True
        net.forward_backward(tiles.cuda(), *TR.pad_targets(ROWS, 2, (H, W), device="cuda"))
        trunk, taps = net.trunk, net.taps
    else:
        groups = TR.ParamGroups()
        trunk = TR.Trunk(groups, dev, scale)
        groups.build()
        trunk.record_taps = True
        feats = trunk.forward(tiles.cuda())
        g = torch.Generator().manual_seed(seed + 1)
        d = [NR.DR._grad_in(g, *f.shape).cuda() for f in feats]
        trunk.backward(d)
        taps = trunk.taps
        taps[23] = {"in": feats, "din": d}
    torch.cuda.synchronize()
    return st, tiles, trunk, taps


@pytest.mark.parametrize("scale,ch,H,W,seed", NR.MODULE_CASES, ids=lambda v: str(v))
def test_each_module_from_its_own_tapped_input_and_gradient(scale, ch, H, W, seed):
    """Every parameterised top-level module of the trunk, run by the references from the input and the gradient the DEVICE fed it inside the net:
    out, dx, dW, dgamma, dbeta and the running statistics against net_ref.module_refs (block_ref's rounded / plain forms over route_ref /
    attn_ref / dw_ref leaves) under block_ref's bound max(FLOOR, 4 x grain), which comes from the two references alone.  The three vacuous
    dbeta quantities of a PSABlock are printed and not asserted.  SPPF's pools read the device's a1 in the rounded form (route_ref.ref_sppf's pin)."""
    TR = _train()
    st, tiles, trunk, taps = _run_case(TR, scale, ch, H, W, seed)
    NR.check_wiring(taps)
    for i in NR.MODULES:
        x = NR.stem_input(tiles) if i == 0 else taps[i]["in"].cpu()
        dy = taps[i]["dout"].cpu()
        pin = None
        if i == 9:
            c = trunk.m[9].cv1.c2
            pin = trunk.m[9].cat[..., :c].float().cpu().permute(0, 3, 1, 2)
        rounded, plain = NR.module_refs(st, i, x, dy, pin)
        got = NR.collect_module(trunk.m[i], i, taps[i]["out"], taps[i]["din"])
        if i == 0:
            rounded.pop("dx"), plain.pop("dx")  # (the stem's input is the image)
        NR.check_module(f"{scale} ch{ch} {H}x{W} model.{i}", got, rounded, plain)


def test_end_to_end_against_plain_fp64_autograd():
    """Figures only, no threshold (depth-23 bf16 error; the wiring and module tests carry the proof): the device trunk's P3 / P4 / P5 and every
    parameter gradient of models 0-22 against ONE plain fp64 autograd graph of the whole trunk (net_ref.trunk_plain), both driven by the
    gradients the device head and criterion returned for P3 / P4 / P5.  yolo11n, 64 x 64, B = 2.  The figures are recorded in DESIGN 3.11."""
    TR = _train()
    scale, ch, H, W, seed = NR.MODULE_CASES[0]
    st, tiles, trunk, taps = _run_case(TR, scale, ch, H, W, seed)
    feats, grads = NR.trunk_plain(st, tiles, [g.cpu() for g in taps[23]["din"]])
    rel = lambda a, b: float((a.double().cpu().reshape(b.shape) - b).abs().max()) / max(float(b.abs().max()), 1e-300)
    for j, k in enumerate(("P3", "P4", "P5")):
        print(f"  end to end {k}: max |d| / max |ref| = {rel(taps[23]['in'][j].permute(0, 3, 1, 2), feats[k]):.3e}")
    fam = {"dW": [], "dgamma": [], "dbeta": []}
    for name, b in trunk.named_blocks():
        inv = None
        if name.endswith("attn.qkv"):
            inv = torch.argsort(TR.qkv_device_order(b.c1 // 64))
        for k, t in (("dW", b.dw), ("dgamma", b.dgamma), ("dbeta", b.dbeta)):
            t = t.cpu() if inv is None else t.cpu()[inv]
            if not f"{name}.{k}".endswith(NR.VACUOUS):
                fam[k].append((rel(t, grads[f"{name}.{k}"]), name))
    for k, v in fam.items():
        v.sort()
        print(f"  end to end {k}: median {v[len(v) // 2][0]:.3e}, worst {v[-1][0]:.3e} ({v[-1][1]}), best {v[0][0]:.3e} ({v[0][1]}) over {len(v)} layers")
    _, routs = NR.ref_module_inputs(st, tiles)  # the ROUNDED reference chained on the CPU: how far bf16 storage alone sits from plain fp64
    for j, t in enumerate(NR.HEAD_FROM):
        print(f"  rounded reference P{3 + j}: max |d| / max |ref| = {rel(routs[t].permute(0, 3, 1, 2), feats[f'P{3 + j}']):.3e}")
    assert all(len(v) >= 60 for v in fam.values())


def test_stale_plan_is_refused():
    """After an optimiser step the packed weights are stale: a forward driven by hand raises until the plan has run again."""
    TR = _train()
    net = TR.Net.from_state(_state("n", 3, seed=51), "n", 12, 3)
    tiles, gt = _tiles(64, 64, 3), TR.pad_targets(ROWS, 2, (64, 64), device="cuda")
    net.step(tiles, *gt)
    with pytest.raises(RuntimeError, match="stale"):
        net.trunk.forward(tiles)
    net.plan.run()
    net.trunk.forward(tiles)
    assert bool(torch.isfinite(net.forward_backward(tiles, *gt)).all())
