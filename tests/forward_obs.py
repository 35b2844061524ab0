"""What one forward of the engine lets a test observe (test_gpu_forward_elems.py, test_gpu_forward_variants.py; the layout helpers also serve
test_forward_variants_cpu.py).  Plain module, no fixtures: `ops` is handed in, so nothing here touches the GPU unless a caller does.

`observe` reads back every tensor ops.debug_activation knows in the plan under test, in the oracle's NCHW channel order, and slices the head
tensor [B, A, >= 65 + nc] into the nine final convs' outputs; forward_ref.Evaluator forms its groups from exactly that."""
import numpy as np
import torch

import bounds
import forward_ref as fr

# Thin, odd and maximal tile shapes (h, w, B) of test_gpu_forward_shapes.py / test_forward_shapes_cpu.py.  LetterBox(auto=True) pads a ragged
# border crop only to the next multiple of 32, so a 10 x 416 crop IS a 32 x 416 network input; the engine accepts every multiple of 32 up to 1280.
SHAPE_TABLE = (
    (32, 32, 70),    # every map <= 16 x 16, the stride-32 map 1 x 1; B neither a multiple of NI nor below it: a partial last whole-image tile
    (32, 64, 5),     # a side of one with H != W
    (64, 32, 5),     # transposed
    (32, 416, 3),    # the thin tile the tiler really makes: the width-keyed fused forms at their minimum heights
    (416, 32, 3),    # its transpose: maps 1 .. 16 wide, none of the width-keyed forms applies
    (64, 416, 2),    # model.17 (4 x 26) on one 4-row stripe of the stride-2 stripe form; at 32 x 416 that is model.3 (4 x 52)
    (96, 96, 3),     # odd stride-32 side (3 x 3); stride-8 map 12 x 12: the 8 x 8 tile, partial both ways
    (160, 160, 2),   # odd stride-32 side (5 x 5); stride-8 map 20 x 20: the 8 x 16 tile, partial both ways
    (32, 1280, 1),   # the engine's maximum side: the stem stripes decline (Win > 416), several column tiles per row
    (1280, 32, 1),   # transposed
)

# Named tensors that are overwritten in place by the time the forward returns.  A tabled name is used neither as input nor as output: the
# groups around it extend across it with propagated E.  (netplan.hip, Builder)
#   model.10.cv1 (b half), model.10.m.0.attn.proj
#       build(): `conv(nm + ".attn.proj", whole(po), H32, W32, bsl, bsl);  // x = x + attn(x), in place on the b half` and
#                `conv(nm + ".ffn.1", whole(ff), H32, W32, bsl, bsl);      // x = x + ffn(x)`: the b half of psa.ab is written by cv1, by
#       attn.proj and by ffn.1; only the last (ffn.1) survives.  The a half is read back as "model.10.a".
#   <C3k>.cv1 where cv1|cv2 run as one merged launch
#       c3k(): "cv1 and cv2 read the same tensor: one launch writes [a | b]; the last Bottleneck later overwrites the (then dead) `a`
#       member, so the same buffer is cv3's concat input."  (<C3k>.m.1.cv2 is that same slot and is what survives.)
STALE_ALWAYS = ("model.10.cv1", "model.10.m.0.attn.proj")
C3K_BLOCKS = ("model.6.m.0", "model.8.m.0", "model.22.m.0")


def _stale(plan):
    return set(STALE_ALWAYS) | {b + ".cv1" for b in C3K_BLOCKS if any(f"{b}.cv1|{b}.cv2" in l for l in plan)}


def _nchw(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def head_width(m):
    """the specified columns of a head row: [64 box | nc class | 1 angle]; the device pads rows to a multiple of 4 floats"""
    return 65 + m.nc


def head_width_padded(m):
    return (head_width(m) + 3) // 4 * 4


def qkv_to_oracle(m, t):
    """NCHW qkv tensor in the device's channel order [q heads | k heads | v heads] -> the oracle's per-head [q | k | v] order"""
    nh = m.psa_heads
    hd = m.psa_c // nh
    o = torch.empty_like(t)
    o[:, fr.qkv_device_order(nh, hd // 2, hd)] = t
    return o


def _read(ops, m, name, B, h, w):
    """debug_activation(name) as an NCHW fp64 tensor in the oracle's channel order, or None where the plan has no such tensor"""
    from oriented_object_detection_amd import _lib
    try:
        t = _nchw(ops.debug_activation(name, B, h, w))
    except _lib.ObbHipError as e:
        if "no activation named" not in str(e):  # any other failure must not pass for "hidden" and silently merge groups
            raise
        return None
    if name.endswith(".attn.qkv"):  # device order [q heads | k heads | v heads]
        t = qkv_to_oracle(m, t)
    return t


def _head_obs(m, head, h, w):
    """head [B, A, >= 65 + nc] -> the nine final convs' outputs, NCHW: every specified column of every anchor of every level"""
    obs, off, no = {}, 0, head_width(m)
    for i, s in enumerate((8, 16, 32)):
        H, W = h // s, w // s
        t = _nchw(head[:, off:off + H * W, :no].reshape(head.shape[0], H, W, no))
        off += H * W
        for n, c in zip(fr.head_names(i), ((0, 64), (64, 64 + m.nc), (64 + m.nc, 65 + m.nc))):
            obs[n] = t[:, c[0]:c[1]]
    assert off == head.shape[1]
    return obs


def _observe(ops, m, plan, head, x, B, h, w):
    stale = _stale(plan)
    obs = {"tile": x}
    for name in list(m.convs) + [f"model.10.m.{i}.attn" for i in range(m.psa_n)]:
        t = _read(ops, m, name, B, h, w)
        if t is None:
            continue
        if name == "model.10.cv1":
            obs["model.10.a"] = t[:, :m.psa_c]
        if name not in stale:
            obs[name] = t
    obs.update(_head_obs(m, head.cpu(), h, w))
    return obs


def check_every_group(ops, m, prec, tail, scale, ch, h, w, B, plan_check=None):
    """One forward of `m` at B tiles of h x w, per element against fp64 (module docstring of test_gpu_forward_elems.py): head in a guarded
    buffer, every observable tensor read back, every group through forward_ref.check_all with full coverage asserted, then the replay on a
    side stream bit-identical with the worst group checked again.  plan_check(plan) may assert what the lowered plan contains.
    -> (plan, {group: worst |err| / bound})"""
    ops.model_load(m.to_blob(), precision=prec, tail=tail)
    try:
        plan = ops.debug_plan(h, w)
        label = f"{prec} {'default' if tail else 'tail=False'} {scale} ch{ch} {h}x{w} B{B}: "
        if plan_check is not None:
            plan_check(plan)
        if not tail:
            assert not any(l.startswith(("bneck ", "c3kimg ", "dwpw ", "front ")) or "+model." in l for l in plan), plan
        x = np.random.default_rng(1000 + h + w + B).integers(0, 256, (B, h, w, ch), dtype=np.uint8)
        xd = torch.as_tensor(x).cuda()
        info = ops.model_info(h, w)
        g = bounds.Guarded((B, info["anchors"], 80), torch.float32)
        ops.forward(xd, out=g.out)
        torch.cuda.synchronize()
        assert g.guards_intact(), label + "write outside the head tensor"
        head = g.out.clone()
        assert bool(torch.isfinite(head[..., :77]).all()), label + "head element not written or not finite"

        obs = _observe(ops, m, plan, head, x, B, h, w)
        ev = fr.Evaluator(m, prec, obs)
        outputs = [k for k in obs if k != "tile"]
        ratios, covered = fr.check_all(ev, outputs, label=label)
        # coverage is asserted, not assumed
        assert len(m.convs) == 96 and {c for c in covered if c in m.convs} == set(m.convs), set(m.convs) - covered
        assert {"attn:model.10.m.0.attn", "up:up13", "up:up16", "pool:model.9.pool0", "pool:model.9.pool1", "pool:model.9.pool2"} <= covered, covered
        assert all(n in ratios for i in range(3) for n in fr.head_names(i))
        if not tail:  # every layer observable: nothing but the tabled in-place tensors is missing
            assert set(m.convs) - set(obs) == _stale(plan), set(m.convs) - set(obs)
        worst = max(ratios, key=ratios.get)
        print(f"{label}{len(outputs)} groups, worst ratio {ratios[worst]:.3f} at {worst}", flush=True)

        # replay: the second sighting of (batch, tiles, head) on a side stream is where the engine captures a hipGraph and launches it.
        # (NOT verified here that the graph path was taken: the engine falls back to eager launches silently if capture or instantiation
        #  fails and exposes no counter; test_hipgraph_capture_and_replay has the same limit.  Either way the head must be identical.)
        g.raw.fill_(0xFF)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            ops.forward(xd, out=g.out)
        st.synchronize()
        torch.cuda.synchronize()
        assert g.guards_intact(), label + "replay: write outside the head tensor"
        assert torch.equal(g.out.view(torch.int32), head.view(torch.int32)), label + "replay: head not bit-identical"
        if fr.is_head(worst):
            again = _head_obs(m, g.out.cpu(), h, w)[worst]
        elif worst == "model.10.a":
            again = _read(ops, m, "model.10.cv1", B, h, w)[:, :m.psa_c]
        else:
            again = _read(ops, m, worst, B, h, w)
        ref, E, _ = ev.node(worst)
        fr.check_group(label + "replay " + worst, again, ref, E)
    finally:
        ops.model_load(m.to_blob())
    return plan, ratios
