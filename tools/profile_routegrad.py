"""Times the four gradient-routing ops of csrc/routegrad.hip at the n / s catalogue shapes, B = 16 (profiles/routegrad.md): each op is captured
N times back to back into one torch.cuda.graph, the graph is replayed between two device events; median (min..max) of ROUNDS rounds, per call.

    python tools/profile_routegrad.py [--quick] [OUT.md]      needs the GPU; prints and writes the markdown table"""
import os
import statistics
import sys

import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oriented_object_detection_amd  # noqa
from oriented_object_detection_amd import ops

O = torch.ops.obbhip
N, REPLAYS, ROUNDS = 20, 50, 7
QUICK = "--quick" in sys.argv
if QUICK:
    REPLAYS, ROUNDS = 5, 1


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(gr, stream=st):
            for _ in range(N):
                fn()
    gr.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            gr.replay()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / (N * REPLAYS))
    return statistics.median(ts), min(ts), max(ts)


rows = []
bf = lambda *s: torch.randn(*s, device="cuda").to(torch.bfloat16)
B = 16
for tag, (H, W, C) in {"n SPPF": (13, 13, 128), "s SPPF": (13, 13, 256), "n SPPF 128px": (4, 4, 128)}.items():
    x = bf(B, H, W, C); cat = ops.sppf_pools_fwd_bf16(x); dcat = bf(B, H, W, 4 * C); dx = torch.empty_like(x)
    e = B * H * W * C * 2
    rows.append((f"pools fwd {tag} {B}x{H}x{W}x{C}", 5 * e, timed(lambda: O.sppf_pools_fwd(x, cat))))
    rows.append((f"pools bwd {tag} {B}x{H}x{W}x{C}", 8 * e, timed(lambda: O.sppf_pools_bwd(cat, dcat, dx))))
for tag, (H, W, Ca, Cb, up) in {"n FPN 13": (13, 13, 256, 128, 2), "n FPN 26": (26, 26, 128, 128, 2), "s FPN 13": (13, 13, 512, 256, 2), "s FPN 26": (26, 26, 256, 256, 2),
                                "n PAN 26": (26, 26, 64, 128, 1), "n PAN 13": (13, 13, 128, 256, 1), "s PAN 26": (26, 26, 128, 256, 1), "s PAN 13": (13, 13, 256, 512, 1)}.items():
    a, b = bf(B, H, W, Ca), bf(B, H * up, W * up, Cb)
    out = ops.upcat_fwd_bf16(a, b, up); dout = bf(*out.shape); da, db = torch.zeros_like(a), torch.zeros_like(b)
    nb = (a.numel() + b.numel() + out.numel()) * 2
    rows.append((f"upcat fwd {tag} {B}x{H}x{W} {Ca}+{Cb} up{up}", nb, timed(lambda: O.upcat_fwd(a, b, up, out))))
    rows.append((f"upcat bwd {tag} {B}x{H}x{W} {Ca}+{Cb} up{up}", nb, timed(lambda: O.upcat_bwd(dout, H, W, Ca, up, da, db, False, False))))
    rows.append((f"upcat bwd accum {tag}", nb + (a.numel() + b.numel()) * 2, timed(lambda: O.upcat_bwd(dout, H, W, Ca, up, da, db, True, True))))
paths = [a for a in sys.argv[1:] if not a.startswith("--")]
with open(paths[0] if paths else os.devnull, "w") as f:
    f.write("| op | bytes (floor) | us median (min..max) | GB/s |\n|---|---|---|---|\n")
    for name, nb, (med, lo, hi) in rows:
        line = f"| {name} | {nb} | {med:.2f} ({lo:.2f}..{hi:.2f}) | {nb / med / 1e3:.0f} |"
        print(line); f.write(line + "\n")
