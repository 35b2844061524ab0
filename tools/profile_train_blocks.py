"""Kernel-trace driver for one train.C3k2 forward + backward (profiles/train_blocks.md): what share of the block's kernel time the channel-window
launches (k_chanwin of csrc/routegrad.hip) take.

    rocprofv3 --kernel-trace --stats -d OUT -o model2 -- python tools/profile_train_blocks.py model2
    rocprofv3 --kernel-trace --stats -d OUT -o model6 -- python tools/profile_train_blocks.py model6
    python tools/profile_train_blocks.py --report OUT/.../model2_results.db

    model2   yolo11n model.2 at 416 px, batch 16: 16 x 104 x 104, 32 -> 64, e = 0.25 (c = 16), one Bottleneck member
    model6   yolo11n model.6: 16 x 26 x 26, 128 -> 128, e = 0.5 (c = 64), one C3k member

The report reads the trace (rocprofv3's default SQLite output, view `kernels`), keeps this library's kernels (the block launches nothing else),
drops the warm-up iterations and prints the time per iteration and kernel, the launch counts and k_chanwin's share."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, ITERS = 3, 10
SHAPES = {"model2": (16, 104, 104, 32, 64, 0.25, False), "model6": (16, 26, 26, 128, 128, 0.5, True)}


def run(which):
    sys.path.insert(0, ROOT)
    import torch
    import oriented_object_detection_amd  # noqa: F401
    import oriented_object_detection_amd.train as TR
    B, H, W, c1, c2, e, c3k = SHAPES[which]
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    w = lambda co, ci, k: (torch.randn(co, ci, k, k, device="cuda", generator=g) * (1.5 / (ci * k * k) ** 0.5),)
    c = int(c2 * e)
    bott = lambda a, b: (w(b, a, 3), w(a, b, 3))
    member = (w(c // 2, c, 1), w(c // 2, c, 1), w(c, c, 1), [bott(c // 2, c // 2), bott(c // 2, c // 2)]) if c3k else bott(c, c // 2)
    groups = TR.ParamGroups()
    blk = TR.C3k2(groups, w(2 * c, c1, 1), w(c2, 3 * c, 1), [member], c3k)
    groups.build()
    x = torch.randn(B, H, W, c1, device="cuda", generator=g).to(torch.bfloat16)
    dy = (torch.randn(B, H, W, c2, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    torch.cuda.synchronize()
    for _ in range(WARMUP + ITERS):
        blk.forward(x)
        blk.backward(dy)
    torch.cuda.synchronize()
    print(f"profile_train_blocks: {which} done")


def short(name):
    n = name.split("(")[0].split("<")[0]
    return n.split("::")[-1].split(" ")[-1]


def report(path):
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, start, end from kernels order by start").fetchall()
    ours = [(short(n), (t1 - t0) / 1e3) for n, t0, t1 in rows if short(n).startswith("k_")]
    per, rem = divmod(len(ours), WARMUP + ITERS)
    assert rem == 0 and per > 0, f"{len(ours)} launches do not divide into {WARMUP + ITERS} iterations"
    timed = ours[-ITERS * per:]
    tot, cnt = collections.OrderedDict(), collections.Counter()
    for n, t in timed:
        tot[n] = tot.get(n, 0.0) + t / ITERS
        cnt[n] += 1
    total = sum(tot.values())
    print(f"{per} launches per forward + backward, {total:.1f} us of kernel time (mean of {ITERS} iterations after {WARMUP} warm-up)\n")
    print("| kernel | launches | us per iteration | share |")
    print("|---|---|---|---|")
    for n, t in sorted(tot.items(), key=lambda kv: -kv[1]):
        print(f"| {n} | {cnt[n] // ITERS} | {t:.1f} | {t / total:.1%} |")
    cw = tot.get("k_chanwin", 0.0)
    print(f"\nk_chanwin: {cnt['k_chanwin'] // ITERS} launches, {cw:.1f} us, {cw / total:.1%} of the block's kernel time")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        run(sys.argv[1] if len(sys.argv) > 1 else "model2")
