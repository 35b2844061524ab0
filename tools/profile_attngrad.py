"""Times the attention core of csrc/attngrad.hip at the C2PSA shapes of yolo11 n / s / x, B = 16, N = 169 (416-px tile) and 16 (128-px tile)
(profiles/attngrad.md): forward, backward (with dv_add), and torch's bf16 version of the same three-step formula (matmul, softmax, matmul) on the
same values -- forward, and forward + autograd backward in one captured function.  Method of tools/profile_dwgrad.py: each op is captured N
times back to back into one torch.cuda.graph, the graph is replayed between two device events; median (min..max) of ROUNDS rounds, per call.

    python tools/profile_attngrad.py [--quick] [OUT.md]      needs the GPU; prints and writes the markdown table"""
import os
import statistics
import sys

import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oriented_object_detection_amd  # noqa
from oriented_object_detection_amd import ops  # noqa

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


B, SCALE = 16, 32 ** -0.5
rows = []
for tokens in (169, 16):
    for nh in (2, 4, 6):
        qkv = torch.randn(B, tokens, nh * 128, device="cuda").to(torch.bfloat16)
        dout = (torch.randn(B, tokens, nh * 64, device="cuda") * 0.5).to(torch.bfloat16)
        dv_add = torch.zeros_like(dout)
        out, lse, dqkv = torch.empty_like(dout), torch.empty(B, nh, tokens, device="cuda"), torch.empty_like(qkv)
        t = {"fwd": timed(lambda: O.attn_fwd(qkv, nh, out, lse)), "bwd": timed(lambda: O.attn_bwd(qkv, out, lse, dout, dv_add, nh, dqkv))}
        # torch: the same values as [B, nh, N, d] views of the same buffers
        sp = lambda a, b: qkv[..., a * nh:b * nh].reshape(B, tokens, nh, -1).permute(0, 2, 1, 3)
        q, k, v = (sp(0, 32).detach().requires_grad_(True), sp(32, 64).detach().requires_grad_(True), sp(64, 128).detach().requires_grad_(True))
        dot = dout.reshape(B, tokens, nh, 64).permute(0, 2, 1, 3)
        f = lambda: torch.softmax((q @ k.transpose(-2, -1)) * SCALE, -1) @ v
        with torch.no_grad():
            t["torch fwd"] = timed(f)
        # forward and backward in one captured function (autograd runs a backward op on its forward op's stream)
        t["torch fwd+bwd"] = timed(lambda: torch.autograd.grad(f(), (q, k, v), dot))
        print(f"N {tokens} nh {nh}: " + ", ".join(f"{k_} {v_[0]:.2f}" for k_, v_ in t.items()), flush=True)
        flop = 2.0 * B * nh * tokens * tokens * (32 + 64)  # forward: S and P v
        rows.append((f"{B} x {tokens} x nh {nh}", flop, t))
paths = [a for a in sys.argv[1:] if not a.startswith("--")]
cols = ["fwd", "bwd", "torch fwd", "torch fwd+bwd"]
with open(paths[0] if paths else os.devnull, "w") as fo:
    head = "| B x N x heads | forward MFLOP | " + " | ".join(f"{c} us" for c in cols) + " | torch bwd (difference) us | bwd / torch bwd |\n|" + "---|" * (len(cols) + 4)
    print(head); fo.write(head + "\n")
    for name, flop, t in rows:
        cells = " | ".join(f"{t[c][0]:.2f} ({t[c][1]:.2f}..{t[c][2]:.2f})" for c in cols)
        tb = t["torch fwd+bwd"][0] - t["torch fwd"][0]
        line = f"| {name} | {flop / 1e6:.1f} | {cells} | {tb:.2f} | {t['bwd'][0] / tb:.2f} |"
        print(line); fo.write(line + "\n")
