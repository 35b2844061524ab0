"""Kernel-trace driver for the multiple-of-8 weight gradient (csrc/convgrad.hip, k_conv_wgrad_c8 + k_wgrad_reduce_c8) at narrow catalogue
shapes of YOLO11 n / s, batch 16, next to the 64-wide kernel (k_conv_wgrad + k_wgrad_reduce) at 64 -> 64 on the same 104 x 104 map:

    rocprofv3 --kernel-trace --stats -d OUT -o wgrad_c8 -- python tools/profile_wgrad_c8.py
    python tools/profile_wgrad_c8.py --report OUT/.../wgrad_c8_results.db [OUT.md]

The second form reads the trace (rocprofv3's default SQLite output, view `kernels`).  The calls are issued in a fixed order, WARMUP + ITERS
per shape, and each call is `classes` launches of the main kernel (one per class of blocks) plus one reduce: the report walks the wgrad
kernels of the trace in start order, checks the names against that sequence, drops the warm-up calls and prints the average time per call
with the useful MACs' rate (2 B Ho Wo k^2 cin cout flop; the exact-f32 MFMA peak of the chip is 157 Tflop/s)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 16
WARMUP, ITERS = 2, 5
# (route, k, s, c1, c2, H = W of the input map)
SHAPES = [
    ("c64", 3, 1, 64, 64, 104), ("c8", 3, 1, 64, 64, 104),
    ("c8", 3, 1, 16, 8, 104), ("c8", 3, 1, 8, 16, 104), ("c8", 3, 1, 32, 16, 104), ("c8", 1, 1, 32, 32, 104), ("c8", 1, 1, 48, 64, 104),
    ("c8", 3, 2, 16, 32, 208), ("c8", 3, 2, 32, 64, 208),
    ("c8", 1, 1, 96, 128, 52), ("c8", 3, 1, 64, 16, 52), ("c8", 3, 1, 32, 32, 26), ("c8", 3, 1, 64, 32, 26),
    ("c8", 3, 1, 256, 16, 13), ("c8", 3, 1, 512, 32, 13),
]


def classes(route, c1, c2):
    """Main-kernel launches per call: one per (full | partial cout block) x (full | partial cin block) class that has blocks."""
    if route == "c64":
        return 1
    side = lambda c: (1 if c >= 64 else 0) + (1 if c % 64 else 0)
    return side(c1) * side(c2)


def run():
    sys.path.insert(0, ROOT)
    import torch
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for route, k, s, c1, c2, hw in SHAPES:
        ho = (hw + s - 1) // s
        x = torch.randn(B, hw, hw, c1, device="cuda", generator=g).to(torch.bfloat16)
        dy = torch.randn(B, ho, ho, c2, device="cuda", generator=g).to(torch.bfloat16)
        op = ops.conv_wgrad_bf16 if route == "c64" else ops.conv_wgrad_c8_bf16
        for _ in range(WARMUP + ITERS):
            op(x, dy, k, stride=s)
        torch.cuda.synchronize()
    print("profile_wgrad_c8: done")


def report(path, out=None):
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, start, end from kernels order by start").fetchall()
    rows = [(n, (t1 - t0) / 1e3) for n, t0, t1 in rows if "wgrad" in n]
    lines = ["| kernel | k, s, c1 -> c2 | map | launches per call | main kernel(s) (us) | reduce (us) | call (us) | useful Tflop/s |", "|---|---|---|---|---|---|---|---|"]
    i = 0
    for route, k, s, c1, c2, hw in SHAPES:
        ncls = classes(route, c1, c2)
        c8 = route == "c8"
        is_main = lambda n: "k_conv_wgrad" in n and ("k_conv_wgrad_c8" in n) == c8
        is_red = lambda n: "k_wgrad_reduce" in n and ("k_wgrad_reduce_c8" in n) == c8
        main, red = [], []
        for _ in range(WARMUP + ITERS):
            call = rows[i:i + ncls + 1]
            i += ncls + 1
            assert len(call) == ncls + 1 and all(is_main(n) for n, _ in call[:-1]) and is_red(call[-1][0]), (route, k, s, c1, c2, call)
            main.append(sum(t for _, t in call[:-1]))
            red.append(call[-1][1])
        m, r = sum(main[WARMUP:]) / ITERS, sum(red[WARMUP:]) / ITERS
        ho = (hw + s - 1) // s
        flop = 2.0 * B * ho * ho * k * k * c1 * c2
        lines.append(f"| {'k_conv_wgrad' if route == 'c64' else 'k_conv_wgrad_c8'} | {k}x{k} s{s} {c1} -> {c2} | {B} x {hw} x {hw} | {ncls} + 1 | {m:.1f} | {r:.1f} | "
                     f"{m + r:.1f} | {flop / ((m + r) * 1e-6) / 1e12:.2f} |")
    assert i == len(rows), (i, len(rows))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        open(out, "w").write(text)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        run()
