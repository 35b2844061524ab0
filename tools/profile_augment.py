"""Kernel-trace driver for one training batch built on the device (augment.TrainBatcher.batch; profiles/train_net.md, "The batch in front of it"), by
the method of tools/profile_train_net.py: one `rocprofv3 --kernel-trace --stats` run (no counters in the same run), this library's kernels read from
the tracer's SQLite output, warm-up dropped, mean over the measured iterations.

    rocprofv3 --kernel-trace --stats -d OUT -o aug -- python tools/profile_augment.py run
    python tools/profile_augment.py --report OUT/.../aug_results.db

    workload   416 x 416 x 3 tiles, batch 16 out of a pool of 64 tiles with twelve labels each, the default AugmentConfig (mosaic 1.0, HSV on)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, ITERS = 3, 10
IMG, BATCH, POOL, LABELS = 416, 16, 64, 12


def run():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import aug_ref
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import augment as A
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    tiles = torch.randint(0, 256, (POOL, IMG, IMG, 3), dtype=torch.uint8, generator=g).cuda()
    lab, cnt = aug_ref.label_pool(POOL, LABELS, IMG, seed=0)
    bt = A.TrainBatcher(tiles, torch.from_numpy(lab).cuda(), torch.from_numpy(cnt).cuda(), A.AugmentConfig(), n_cap=64)
    rng = np.random.RandomState(0)
    for it in range(WARMUP + ITERS):
        bt.batch(rng.randint(0, POOL, BATCH), rng)
        torch.cuda.synchronize()
    print(f"profile_augment: done, survivors per tile in the last batch {bt.count.cpu().tolist()}")


def report(path):
    import collections
    import re
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, start, end from kernels order by start").fetchall()
    ours = [(re.search(r"\bk_aug\w*", n).group(0), (t1 - t0) / 1e3) for n, t0, t1 in rows if re.search(r"\bk_aug\w*", n)]
    per, rem = divmod(len(ours), WARMUP + ITERS)
    assert rem == 0 and per > 0, f"{path}: {len(ours)} launches do not divide into {WARMUP + ITERS} batches"
    tot = collections.OrderedDict()
    for n, t in ours[-ITERS * per:]:
        tot[n] = tot.get(n, 0.0) + t / ITERS
    print(f"{IMG} px, batch {BATCH}, 3 channels, mosaic + HSV: {per} launches per batch, mean of {ITERS} batches after {WARMUP} warm-up")
    print("| kernel | us per batch |\n|---|---|")
    for n, t in tot.items():
        print(f"| {n} | {t:.1f} |")
    print(f"| total | {sum(tot.values()):.1f} |")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if len(sys.argv) >= 3 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        run()
