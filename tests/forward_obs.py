"""What one forward of the engine lets a test observe (test_gpu_forward_elems.py, test_gpu_forward_variants.py; the layout helpers also serve
test_forward_variants_cpu.py).  Plain module, no fixtures: `ops` is handed in, so nothing here touches the GPU unless a caller does.

`observe` reads back every tensor ops.debug_activation knows in the plan under test, in the oracle's NCHW channel order, and slices the head
tensor [B, A, >= 65 + nc] into the nine final convs' outputs; forward_ref.Evaluator forms its groups from exactly that."""
import torch

import forward_ref as fr

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
