"""The trainer's validation on the device: the fold kernel bit for bit against numpy float32 (live and EMA buffers, after real trainer steps), the
engine after `Validator`'s reload against a host-written blob and against fp64, training undisturbed by a validation, ops.val_match exactly against
tests/val_ref.py on the cases whose margins tests/test_validate_cpu.py asserts, and `Validator` end to end against its parts chained by hand."""
import numpy as np
import pytest
import torch

import forward_ref as FR
import net_ref as NR
import val_ref as VR
from bounds import Guarded

pytestmark = pytest.mark.gpu


def _mods():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, metrics, model, ops, train
    return _lib, metrics, model, ops, train


def _state(scale, ch, seed):
    return {k: v.cuda() for k, v in NR.make_state(scale, 12, ch, seed=seed).items()}


def _tiles(n, s, ch, seed):
    return torch.randint(0, 256, (n, s, s, ch), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).cuda()


ROWS = [[0, 3, 0.5, 0.5, 0.4, 0.3, 0.2], [0, 1, 0.3, 0.7, 0.3, 0.5, -0.4], [1, 7, 0.4, 0.6, 0.5, 0.5, 1.0]]


def _trainer(TR, net, ema=True):
    e = TR.ModelEMA(net.groups, decay=0.9, tau=2) if ema else None  # (a short horizon: after two updates the EMA has visibly moved)
    net.update = TR.TrainerUpdate(net.groups, TR.Schedule(epochs=3, nb=4, lr0=0.01, batch=2, nbs=2), ema=e)
    return e


def _pool(n, s, ch, seed):
    """a pool of n tiles with 0..3 synthetic labels each: (tiles, labels fp64 [n,4,9], counts)"""
    rng = np.random.RandomState(seed)
    lab, cnt = np.zeros((n, 4, 9)), np.zeros(n, np.int32)
    for i in range(n):
        cnt[i] = i % 4
        for j in range(cnt[i]):
            cx, cy, w, h, t = rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), rng.uniform(0.15, 0.4), rng.uniform(0.15, 0.4), rng.uniform(0, 1.5)
            c, s_ = np.cos(t), np.sin(t)
            pts = [(cx + dx * w / 2 * c - dy * h / 2 * s_, cy + dx * w / 2 * s_ + dy * h / 2 * c) for dx, dy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
            lab[i, j] = [rng.randint(0, 12)] + [v for p in pts for v in p]
    return _tiles(n, s, ch, seed), torch.from_numpy(lab).cuda(), torch.from_numpy(cnt).cuda()


# ------------------------------------------------------------------------------------------------------------ 4. fold bits
def _fold_numpy(net, flats, eps):
    """the data section from host copies of the four flat buffers: the three lines of the fold in numpy float32, qkv rows to checkpoint order.  Every
    offset is read from the BLOCK's own views of the live flat buffers (storage offsets), nothing from the plan under test."""
    live = [o.param for o in net.groups.opts] + [net.groups.buffers]
    w, g, b, buf = (t.cpu().numpy() for t in flats)
    off = lambda t, k: t.storage_offset() - live[k].storage_offset()
    e, out = np.float32(eps), []
    for name, blk in net.named_blocks():
        cout, per = blk.w.shape[0], blk.w[0].numel()
        W = w[off(blk.w, 0):off(blk.w, 0) + cout * per].reshape(cout, per)
        if NR.is_plain(name):
            out += [W.reshape(-1), b[off(blk.b, 2):off(blk.b, 2) + cout]]
            continue
        sl = lambda a, t, k: a[off(t, k):off(t, k) + cout]
        f = sl(g, blk.gamma, 1) / np.sqrt(sl(buf, blk.running_var, 3) + e)
        Wf, bf = W * f[:, None], sl(b, blk.beta, 2) - sl(buf, blk.running_mean, 3) * f
        assert f.dtype == Wf.dtype == bf.dtype == np.float32
        if name.endswith("attn.qkv"):
            inv = np.argsort(np.asarray(FR.qkv_device_order(cout // 128, 32, 64)))  # checkpoint row c sits in device row inv[c]
            Wf, bf = Wf[inv], bf[inv]
        out += [Wf.reshape(-1), bf]
    return np.concatenate(out)


@pytest.mark.parametrize("scale,ch", [("n", 3), ("n", 4), ("s", 3)], ids=["n-ch3", "n-ch4", "s-ch3"])
def test_fold_kernel_bits(scale, ch):
    _lib, _, _, ops, TR = _mods()
    net = TR.Net.from_state(_state(scale, ch, seed=21), scale, 12, ch)
    ema = _trainer(TR, net)
    before = [t.clone() for t in ema.live()]
    gt = TR.pad_targets(ROWS, 2, (64, 64), device="cuda")
    for ni in range(2):
        net.step(_tiles(2, 64, ch, 30 + ni), *gt, ni=ni, epoch=0)
    assert all(not torch.equal(a, b) for a, b in zip(before, ema.live())) and all(not torch.equal(a, b) for a, b in zip(ema.live(), ema.ema))
    plan = TR.FoldPlan(net)
    fold = net.fold()
    for what, flats, e in (("live", ema.live(), None), ("ema", ema.ema, ema)):
        ref = torch.from_numpy(_fold_numpy(net, flats, plan.eps))
        g = Guarded((plan.table.out_elems,), torch.float32)
        ops.fold_blob_f32(*flats, plan.table, plan.eps, out=g.out)
        got = g.get(f"fold {what}").cpu()
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), what
        blob = bytes(plan.run(e))
        assert torch.equal(torch.frombuffer(bytearray(blob[plan.data_off:]), dtype=torch.float32).view(torch.int32), ref.view(torch.int32)), what
    # the live fold is Net.fold() bit for bit, EVERY record (names in blob order): in particular the qkv rows are in checkpoint order
    got = plan.fold().cpu()
    o = 0
    for name in plan.names:
        w, b = fold[name]
        n = w.numel()
        assert torch.equal(got[o:o + n].view(torch.int32), w.detach().cpu().reshape(-1).view(torch.int32)), name
        assert torch.equal(got[o + n:o + n + b.numel()].view(torch.int32), b.detach().cpu().contiguous().view(torch.int32)), name
        o += n + b.numel()
    assert o == got.numel()
    # a table of another plan: wrong nrec, wrong out_elems -> nothing is written
    H, R = _lib.FOLD_TABLE_HEAD, _lib.FOLD_TABLE_REC
    tab, nrec, flats = plan.table.table, plan.table.nrec, ema.live()
    g = Guarded((plan.table.out_elems,), torch.float32)
    torch.ops.obbhip.fold_blob(*flats, tab[:H + (nrec - 1) * R], nrec - 1, plan.eps, g.out)
    torch.ops.obbhip.fold_blob(*flats, tab, nrec, plan.eps, g.out[:-1])
    torch.cuda.synchronize()
    assert bool((g.raw == 0xFF).all())
    with pytest.raises(_lib.ObbHipError):
        torch.ops.obbhip.fold_blob(*flats, tab, nrec - 1, plan.eps, g.out)  # the table's length does not fit nrec: refused on the host
    torch.cuda.synchronize()
    assert bool((g.raw == 0xFF).all())


# ------------------------------------------------------------------------------------------------------------ 5. engine parity
def _host_blob(net, scale, ch):
    from tools.export_obbw import blob_from_records
    t = NR.conv_table(scale, net.nc, ch)
    return blob_from_records([(n, t[n].c1, t[n].c2, t[n].k, t[n].s, t[n].g, t[n].act, w.detach().cpu(), b.detach().cpu()) for n, (w, b) in net.fold().items()],
                             net.nc, ch, scale)


def _oracle_like(scale, nc, ch, fold):
    """an oracle model object (graph and channel arithmetic only) carrying the folded weights: what forward_ref's Evaluator takes"""
    from oracle.yolo11_obb import SCALES, Yolo11OBB
    m = Yolo11OBB.__new__(Yolo11OBB)
    m.scale, m.nc, m.ch = scale, nc, ch
    m.depth, m.width, m.max_ch = SCALES[scale]
    m.convs = {}
    m._define()
    for name, r in m.convs.items():
        r.w, r.b = fold[name][0].detach().cpu().float(), fold[name][1].detach().cpu().float()
    return m


def test_engine_parity_after_reload():
    _lib, _, _, ops, TR = _mods()
    import forward_obs as FO
    # a net whose fold IS a calibrated oracle model (activations O(1) through all layers): the scale test_gpu_fp32.py's absolute caps are set for
    from oracle.yolo11_obb import Yolo11OBB
    net = TR.Net.from_state({k: t.cuda() for k, t in NR.state_of_oracle(Yolo11OBB("n", nc=12, ch=3, seed=3)).items()}, "n", 12, 3)
    pool = _pool(2, 64, 3, seed=40)
    v = TR.Validator(net, pool, batch=2)
    slot0 = ops.get_option("model_slot")
    v()
    assert ops.get_option("model_slot") == slot0
    assert torch.equal(v.tiles, pool[0])  # what the engine read: the pool's tiles, byte for byte
    tiles = pool[0]
    fold = {k: (w.detach().cpu(), b.detach().cpu()) for k, (w, b) in net.fold().items()}
    m = _oracle_like("n", 12, 3, fold)
    x = tiles.cpu().numpy()
    with ops.engine_state():
        v.model._ensure_active()
        head = ops.forward(tiles).clone()
        obs = FO._observe(ops, m, ops.debug_plan(64, 64), head, x, 2, 64, 64)
        ops.select_model(63)
        ops.model_load(_host_blob(net, "n", 3), precision="f32")
        ref_head = ops.forward(tiles).clone()
        ops.model_unload(63)
    assert torch.equal(head.view(torch.int32), ref_head.view(torch.int32))
    # per element against fp64 under forward_ref's bound for the fp32 plan, as test_gpu_forward_elems.py applies it: every observable tensor of the
    # reloaded model against its group evaluated in fp64 from the FOLDED weights, all 96 convs inside checked groups
    ev = FR.Evaluator(m, "f32", obs)
    ratios, covered = FR.check_all(ev, [k for k in obs if k != "tile"], label="reloaded f32 n 64x64: ")
    assert {c for c in covered if c in m.convs} == set(m.convs) and all(n in ratios for i in range(3) for n in FR.head_names(i))
    # the head per element against the independent fp64 statement of the whole graph (net_ref.eval_forward) under the yardstick test_gpu_fp32.py
    # (test_fp32_head_matches_fp32_oracle) applies to the fp32 plan end to end, figures unchanged: the device sits as close to fp64 as torch's own
    # fp32 evaluation of the same graph and weights does (largest element within 2 x, mean within 1.5 x), and inside that test's absolute caps
    dev = head.cpu()[..., :77]
    ref64 = NR.eval_forward(fold, x, 12)
    ref32 = m.forward_raw(x, "fp32")
    assert ref64.shape == dev.shape == ref32.shape
    d = (dev - ref32).abs()
    conf_d = (torch.sigmoid(dev[..., 64:76]) - torch.sigmoid(ref32[..., 64:76])).abs()
    e_dev, e_ref = (dev.double() - ref64).abs(), (ref32.double() - ref64).abs()
    print("reloaded f32 n 64x64 vs torch fp32: logit max/mean", float(d.max()), float(d.mean()), "conf max", float(conf_d.max()),
          "| vs fp64 eval_forward: device max/mean", float(e_dev.max()), float(e_dev.mean()), "torch-fp32 max/mean", float(e_ref.max()), float(e_ref.mean()))
    assert float(e_dev.mean()) <= 1.5 * float(e_ref.mean()) + 1e-7 and float(e_dev.max()) <= 2.0 * float(e_ref.max()) + 1e-6
    assert float(d.max()) < 2e-3 and float(d.mean()) < 5e-5 and float(conf_d.max()) < 2e-4


# ------------------------------------------------------------------------------------------------------------ 6. training undisturbed
def test_training_bit_identical_after_validation():
    _, _, _, ops, TR = _mods()
    pool = _pool(3, 64, 3, seed=41)
    gt = TR.pad_targets(ROWS, 2, (64, 64), device="cuda")
    results = []
    for validate in (False, True):
        net = TR.Net.from_state(_state("n", 3, seed=23), "n", 12, 3)
        ema = _trainer(TR, net)
        net.step(_tiles(2, 64, 3, 50), *gt, ni=0, epoch=0)
        if validate:
            out = net.validate(pool, batch=2, ema=ema)
            assert set(out) == {"map50", "map", "fitness", "ap", "n_det", "n_gt"} and out["n_gt"] == int(pool[2].sum())
        net.step(_tiles(2, 64, 3, 51), *gt, ni=1, epoch=0)
        torch.cuda.synchronize()
        results.append([t.clone() for t in ema.live() + ema.ema + [o.grad for o in net.groups.opts] + [s for o in net.groups.opts for s in o.state]])
    assert len(results[0]) == len(results[1])
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ 7. ops.val_match
def _dev(case):
    det, count, gl, gb, mk, nc = case
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (det, count, gl, gb, mk)] + [nc]


@pytest.mark.parametrize("which", ["cases", "tiny"])
def test_val_match_exact(which):
    _lib, _, _, ops, _ = _mods()
    case = VR.match_cases() if which == "cases" else VR.tiny_case()
    band, _ = VR.all_band()  # over every committed case, those of test_gpu_batch_edges.py included
    det, count, gl, gb, mk, nc = case
    B, M = det.shape[:2]
    if which == "cases":
        assert (B, M, gl.shape[1]) == (4, 300, 64) and sorted(count.tolist()) == [0, 1, 7, 300] and sorted(mk.sum(1).tolist()) == [0, 1, 5, 64]
    ref_tp, ref_bi, ref_bg = VR.match(*case)
    outs = (Guarded((B, M), torch.uint16, init=None), Guarded((B, M), torch.float32), Guarded((B, M), torch.int32))
    d = _dev(case)
    ops.val_match(*d, out=tuple(g.out for g in outs))
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in outs)
    tp, bi, bg = (g.out.cpu().numpy() for g in outs)
    assert np.array_equal(bg, ref_bg)
    assert np.array_equal(tp, ref_tp), np.argwhere(tp != ref_tp)[:8]
    print(f"val_match {which}: max |best_iou - fp64| = {np.abs(bi - ref_bi).max():.3e}, band {band:.3e}")
    assert np.abs(bi.astype(np.float64) - ref_bi).max() <= band
    assert ref_tp.any() and (which == "tiny" or (ref_tp[0] == 0x3ff).any())
    # refusals leave the sentinel-filled outputs untouched
    for bad in ("n_cap", "max_det", "null"):
        for g in outs:
            g.raw.fill_(0xFF)
        c, thr = ops.ctx(), ops.val_thresholds("cuda")
        args = [ops._p(t) for t in d[:5]] + [B, M, gl.shape[1], nc, ops._p(thr), 10] + [ops._p(g.out) for g in outs] + [ops._stream()]
        if bad == "n_cap":
            args[7] = 513
        elif bad == "max_det":
            args[6] = 0
        else:
            args[3] = None
        assert _lib.lib().obb_val_match(c, *args) != 0
        rc0 = _lib.lib().obb_val_match(c, *(args[:7] + [0] + args[8:])) if bad == "n_cap" else 1
        assert rc0 != 0
        torch.cuda.synchronize()
        assert all(bool((g.raw == 0xFF).all()) for g in outs), bad


# ------------------------------------------------------------------------------------------------------------ 8. end to end
def test_validator_end_to_end():
    _, metrics, model, ops, TR = _mods()
    net = TR.Net.from_state(_state("n", 3, seed=24), "n", 12, 3)
    ema = _trainer(TR, net, ema=False)
    pool = _pool(6, 64, 3, seed=42)
    v = TR.Validator(net, pool, batch=4, conf=0.001)
    out = v()
    assert v.is_best and v.best_fitness == out["fitness"]
    # the same by hand: host blob -> YOLO -> predict_tiles -> val_match -> ap_per_class, the targets from the labels' own kernel
    with ops.engine_state():
        y = model.YOLO(_host_blob(net, "n", 3), imgsz=64, precision="f32")
        det, count = y.predict_tiles(pool[0], 0.001, 0.7, 300)
        y.close()
    from oriented_object_detection_amd import augment
    tb = augment.TrainBatcher(*pool, cfg=v.batcher.cfg, n_cap=64, bgr=True, swap_rb=False)
    params = np.zeros(6, augment.REC)
    for i in range(6):
        augment.make_record(params[i], np.eye(3), 1.0, 64, src=(i, 0, 0, 0))
    tiles, gl, gb, mk = tb.batch(list(range(6)), None, params=params)
    assert torch.equal(tiles, pool[0])
    tp, _, _ = ops.val_match(det, count, gl, gb, mk, 12)
    live = (torch.arange(300)[None, :] < count.cpu()[:, None]).numpy()
    bits = tp.cpu().numpy()[live]
    tpb = ((bits[:, None].astype(np.int64) >> np.arange(10)[None, :]) & 1).astype(bool)
    ref = metrics.ap_per_class(tpb, det[..., 4].cpu().numpy()[live], det[..., 5].cpu().numpy()[live], gl.cpu().numpy()[mk.cpu().numpy().astype(bool)], 12)
    assert out["n_det"] == int(live.sum()) > 0 and out["n_gt"] == int(pool[2].sum())
    assert np.array_equal(out["ap"], ref["ap"]) and out["map50"] == ref["map50"] and out["map"] == ref["map"] and out["fitness"] == ref["fitness"]
    # detections that ARE the targets: a perfect detector scores 0.995
    n = int(mk.sum(1).max())
    pdet = torch.zeros((6, max(n, 1), 7), device="cuda")
    pdet[:, :n, :4], pdet[:, :n, 6], pdet[:, :n, 5], pdet[:, :n, 4] = gb[:, :n, :4], gb[:, :n, 4], gl[:, :n].float(), 0.9
    v.reset()
    v.update(pdet, mk.sum(1).to(torch.int32), gl, gb, mk)
    perfect = v.result()
    assert abs(perfect["map"] - 0.995) <= 1e-12 and abs(perfect["map50"] - 0.995) <= 1e-12
    # a tile with more labels than n_cap raises instead of losing ground truth (the pool has tiles with three labels)
    small = TR.Validator(net, pool, batch=4, n_cap=2)
    with pytest.raises(ValueError, match="n_cap"):
        small()
    small.close()
    # a second call after another training step: is_best follows the two fitness values
    gt = TR.pad_targets(ROWS, 2, (64, 64), device="cuda")
    net.step(_tiles(2, 64, 3, 60), *gt, ni=0, epoch=0)
    out2 = v()
    assert v.is_best == (out2["fitness"] >= out["fitness"]) and v.best_fitness == max(out["fitness"], out2["fitness"])
