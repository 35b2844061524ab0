"""Kernel-trace driver for the training-mode Conv block kernels at 16 x 104 x 104 x 128 (the BatchNorm of model.3's input level of yolo11s at
416 px, batch 16) and the stride-2 128 -> 128 conv on the same map (model.3):

    rocprofv3 --kernel-trace --stats -d OUT -o train_bn -- python tools/profile_train_bn.py
    python tools/profile_train_bn.py --report OUT/.../train_bn_results.db

The second form reads the trace (rocprofv3's default SQLite output, view `kernels`), drops the warm-up rounds and turns the average kernel
times into achieved bandwidth for the bytes each kernel must move (HBM peak 8.0 TB/s, spec).  The 44 MB tensors fit in the 256 MiB
Infinity Cache, so repeated rounds may be served from it: the fractions are of the HBM rate, not a claim that HBM was the source."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, C = 16, 104, 104, 128
HO, WO = (H + 1) // 2, (W + 1) // 2
NPIX = B * H * W
MB = NPIX * C * 2                 # one bf16 [npix][C] tensor
MB_S2 = B * HO * WO * C * 2       # the stride-2 output
PEAK = 8.0e12

# bytes each kernel must move (reads + writes of the [npix][C]-sized tensors; per-channel vectors and slabs are negligible), keyed by
# (kernel, grid size x): the forward and the dgrad conv are the same k_conv_igemm instantiation
WARMUP, ITERS = 2, 10


def bytes_of(name, grid):
    table = {
        "k_bn_stats_part": MB,            # z once (the block's second, centred pass is served from cache)
        "k_bn_stats_final": 0,
        "k_bn_silu_apply": 2 * MB,        # z in, a out
        "k_bn_bwd_part": 2 * MB,          # z, da
        "k_bn_bwd_final": 0,
        "k_bn_bwd_apply": 3 * MB,         # z, da in, dz out
        "k_zero_insert_s2": MB_S2 + MB,   # dy in, dY_up out
        "k_conv_wgrad": MB + MB_S2,       # x, dy (compute-bound: 2 x 9 x C^2 MACs per output pixel)
        "k_wgrad_reduce": 0,
    }
    for k, v in table.items():
        if k in name:
            return k, v
    if "k_conv_igemm" in name:  # the stride-2 forward reads x, writes y; the dgrad conv reads dY_up, writes dx
        return ("k_conv_igemm (s2 forward)", MB + MB_S2) if grid < 3 * 131072 else ("k_conv_igemm (dgrad, stride 1 on dY_up)", 2 * MB)
    return None, None


def run(iters=ITERS):
    sys.path.insert(0, ROOT)
    import torch
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn(B, H, W, C, device="cuda", generator=g).to(torch.bfloat16)
    da = (torch.randn(B, H, W, C, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    w = torch.randn(C, C, 3, 3, device="cuda", generator=g) * 0.03
    dy = torch.randn(B, HO, WO, C, device="cuda", generator=g).to(torch.bfloat16)
    pk, pkd = ops.conv_pack_bf16(w, H, W, stride=2), ops.conv_pack_bf16(w, H, W, dgrad_form=True)
    for _ in range(iters + WARMUP):
        a, m, inv = ops.bn_silu_fwd_bf16(z, gamma, beta, rm, rv)
        ops.bn_silu_bwd_bf16(z, da, gamma, beta, m, inv)
        ops.conv_fwd_bf16(z, pk, None, C, 3, stride=2)
        ops.conv_dgrad_s2_bf16(dy, pkd, C, H, W)
        ops.conv_wgrad_bf16(z, dy, 3, stride=2)
    torch.cuda.synchronize()
    print("profile_train_bn: done")


def report(path):
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, start, end, grid_x from kernels order by start").fetchall()
    runs = collections.OrderedDict()
    for name, t0, t1, gx in rows:
        key, by = bytes_of(name, gx)
        if key is not None:
            runs.setdefault(key, (by, []))[1].append((t1 - t0) / 1e3)
    print("| kernel | calls timed | avg time (us) | bytes it must move (MB) | achieved (TB/s) | of 8.0 TB/s |")
    print("|---|---|---|---|---|---|")
    for key, (by, ts) in runs.items():
        ts = ts[-ITERS:]
        t_us = sum(ts) / len(ts)
        if by == 0:
            print(f"| {key} | {len(ts)} | {t_us:.1f} | (slab only) | - | - |")
            continue
        bw = by / (t_us * 1e-6)
        print(f"| {key} | {len(ts)} | {t_us:.1f} | {by / 1e6:.1f} | {bw / 1e12:.2f} | {bw / PEAK:.0%} |")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        run()
