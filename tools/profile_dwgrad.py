"""Times the depthwise 3x3 ops of csrc/dwgrad.hip at the nine n / s catalogue shapes, B = 16 (profiles/dwgrad.md): forward, the fused backward,
the backward with dx alone and with dw alone, and the same op through torch.nn.functional.conv2d(groups=C) in bf16 channels-last (forward, and
forward + the autograd backward of both gradients in one captured function) on the same device.  Method of tools/profile_routegrad.py: each op is captured N times back to back
into one torch.cuda.graph, the graph is replayed between two device events; median (min..max) of ROUNDS rounds, per call.

    python tools/profile_dwgrad.py [--quick] [OUT.md]      needs the GPU; prints and writes the markdown table"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F
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


# (layer, H, W, C): model.10.m.0.attn.pe and model.23.cv3.{0,1,2}.{0,1}.0 of yolo11n / yolo11s at 416 px
SHAPES = [("n pe", 13, 13, 128), ("n cv3.0", 52, 52, 64), ("n cv3.1.0", 26, 26, 128), ("n cv3.1.1", 26, 26, 64), ("n cv3.2.0", 13, 13, 256), ("n cv3.2.1", 13, 13, 64),
          ("s cv3.0", 52, 52, 128), ("s cv3.1.0 / pe", 26, 26, 256), ("s cv3.2.0", 13, 13, 512)]
B = 16
rows = []
for tag, H, W, C in SHAPES:
    x = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
    dz = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
    w = torch.randn(C, 1, 3, 3, device="cuda") * 0.3
    z, dx, dw = torch.empty_like(x), torch.empty_like(x), torch.empty_like(w)
    e = x.numel() * 2  # bytes of one tensor
    t = {"fwd": timed(lambda: O.dwconv3_fwd(x, w, z)), "bwd": timed(lambda: O.dwconv3_bwd(x, dz, w, dx, dw)),
         "dx": timed(lambda: O.dwconv3_bwd(x, dz, w, dx, None)), "dw": timed(lambda: O.dwconv3_bwd(x, dz, w, None, dw))}
    # torch: the same tensors as NCHW views in channels-last memory (the NHWC buffers themselves), bf16 weights
    xt, dzt, wt = x.permute(0, 3, 1, 2), dz.permute(0, 3, 1, 2), w.to(torch.bfloat16).requires_grad_(True)
    xg = xt.detach().requires_grad_(True)
    t["torch fwd"] = timed(lambda: F.conv2d(xt, wt.detach(), padding=1, groups=C))
    # forward and backward in one captured function: autograd runs a backward op on the stream of its forward op, so a forward recorded outside
    # the capture would put the backward on a stream the capture does not own
    t["torch fwd+bwd"] = timed(lambda: torch.autograd.grad(F.conv2d(xg, wt, padding=1, groups=C), (xg, wt), dzt))
    print(f"{tag}: " + ", ".join(f"{k} {v[0]:.2f}" for k, v in t.items()), flush=True)
    rows.append((f"{tag} {B}x{H}x{W}x{C}", e, t))
paths = [a for a in sys.argv[1:] if not a.startswith("--")]
cols = ["fwd", "bwd", "dx", "dw", "torch fwd", "torch fwd+bwd"]
with open(paths[0] if paths else os.devnull, "w") as f:
    head = "| shape | bytes: fwd 2e, fused 3e, dx 2e, dw 2e | " + " | ".join(f"{c} us" for c in cols) + " | fused / (dx + dw) | fused GB/s |\n|" + "---|" * (len(cols) + 4)
    print(head); f.write(head + "\n")
    for name, e, t in rows:
        cells = " | ".join(f"{t[c][0]:.2f} ({t[c][1]:.2f}..{t[c][2]:.2f})" for c in cols)
        line = f"| {name} | {2 * e} / {3 * e} / {2 * e} / {2 * e} | {cells} | {t['bwd'][0] / (t['dx'][0] + t['dw'][0]):.2f} | {3 * e / t['bwd'][0] / 1e3:.0f} |"
        print(line); f.write(line + "\n")
