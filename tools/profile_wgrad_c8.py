"""Kernel-trace driver for the dense weight gradient (csrc/convgrad.hip, k_conv_wgrad + k_wgrad_reduce) at batch 16: the narrow catalogue
shapes of YOLO11 n / s, three shapes at multiples of 64, and 3x3 64 -> 64 through both public entries (ops.conv_wgrad_bf16 and
ops.conv_wgrad_c8_bf16 are checks in front of the same launcher):

    rocprofv3 --kernel-trace --stats -d OUT -o wgrad -- python tools/profile_wgrad_c8.py
    python tools/profile_wgrad_c8.py --report OUT/.../wgrad_results.db [OUT.md]

The second form reads the trace (rocprofv3's default SQLite output, view `kernels`).  The calls are issued in a fixed order, WARMUP + ITERS
per shape, and each call is `classes` launches of the main kernel (one per class of blocks) plus one reduce: the report walks the wgrad
kernels of the trace in start order, checks main / reduce against that sequence, drops the warm-up calls and prints, per shape, the median
time of the main kernel(s) and of the reduce with the useful MACs' rate (2 B Ho Wo k^2 cin cout flop; the exact-f32 MFMA peak of the chip is
157 Tflop/s).  Kernels are told apart by shape, not by name, so a trace of an older library (OBB_LIB) reads the same way."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 16
WARMUP, ITERS = 2, 5
# (entry, k, s, c1, c2, H = W of the input map); entry "c64": ops.conv_wgrad_bf16 (multiples of 64 only), "c8": ops.conv_wgrad_c8_bf16
SHAPES = [
    ("c64", 3, 1, 64, 64, 104), ("c8", 3, 1, 64, 64, 104), ("c64", 3, 2, 64, 128, 104), ("c64", 1, 1, 128, 128, 52),
    ("c8", 3, 1, 16, 8, 104), ("c8", 3, 1, 8, 16, 104), ("c8", 3, 1, 32, 16, 104), ("c8", 1, 1, 32, 32, 104), ("c8", 1, 1, 48, 64, 104),
    ("c8", 3, 2, 16, 32, 208), ("c8", 3, 2, 32, 64, 208),
    ("c8", 1, 1, 96, 128, 52), ("c8", 3, 1, 64, 16, 52), ("c8", 3, 1, 32, 32, 26), ("c8", 3, 1, 64, 32, 26),
    ("c8", 3, 1, 256, 16, 13), ("c8", 3, 1, 512, 32, 13),
]


def classes(c1, c2):
    """Main-kernel launches per call: one per (full | partial cout block) x (full | partial cin block) class that has blocks."""
    side = lambda c: (1 if c >= 64 else 0) + (1 if c % 64 else 0)
    return side(c1) * side(c2)


def run():
    sys.path.insert(0, ROOT)
    import torch
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for entry, k, s, c1, c2, hw in SHAPES:
        ho = (hw + s - 1) // s
        x = torch.randn(B, hw, hw, c1, device="cuda", generator=g).to(torch.bfloat16)
        dy = torch.randn(B, ho, ho, c2, device="cuda", generator=g).to(torch.bfloat16)
        op = ops.conv_wgrad_bf16 if entry == "c64" else ops.conv_wgrad_c8_bf16
        for _ in range(WARMUP + ITERS):
            op(x, dy, k, stride=s)
        torch.cuda.synchronize()
    print("profile_wgrad_c8: done")


def measure(path):
    """[(shape, launches of the main kernel per call, median main kernel(s) us, median reduce us)] of one trace, in SHAPES order."""
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, start, end from kernels order by start").fetchall()
    rows = [(n, (t1 - t0) / 1e3) for n, t0, t1 in rows if "wgrad" in n]
    out, i = [], 0
    for shape in SHAPES:
        ncls = classes(shape[3], shape[4])
        main, red = [], []
        for _ in range(WARMUP + ITERS):
            call = rows[i:i + ncls + 1]
            i += ncls + 1
            assert len(call) == ncls + 1 and all("k_conv_wgrad" in n for n, _ in call[:-1]) and "k_wgrad_reduce" in call[-1][0], (shape, call)
            main.append(sum(t for _, t in call[:-1]))
            red.append(call[-1][1])
        out.append((shape, ncls, statistics.median(main[WARMUP:]), statistics.median(red[WARMUP:])))
    assert i == len(rows), (i, len(rows))
    return out


def report(path, out=None):
    lines = ["| k, s, c1 -> c2 | map | entry | launches per call | main kernel(s) (us) | reduce (us) | call (us) | useful Tflop/s |", "|---|---|---|---|---|---|---|---|"]
    for (entry, k, s, c1, c2, hw), ncls, m, r in measure(path):
        ho = (hw + s - 1) // s
        flop = 2.0 * B * ho * ho * k * k * c1 * c2
        lines.append(f"| {k}x{k} s{s} {c1} -> {c2} | {B} x {hw} x {hw} | {'conv_wgrad_bf16' if entry == 'c64' else 'conv_wgrad_c8_bf16'} | {ncls} + 1 | {m:.1f} | {r:.1f} | "
                     f"{m + r:.1f} | {flop / ((m + r) * 1e-6) / 1e12:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        open(out, "w").write(text)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        run()
