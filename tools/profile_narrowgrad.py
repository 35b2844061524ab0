"""Times the narrow kernels against the zero-padded dense route at the workload shapes (batch 16).  Device events, alternating A / B.  The padded
route keeps its padded weights and bias resident (padded rows in the optimiser's buffers): per call it pays the activation / dy pad, the pack, the
dense kernels and the slice.
  --kernels PLAN.json        no timing: 20 calls of each new op per shape, the plan (label, launches per call) written for --parse; run it under
                             `rocprofv3 --kernel-trace` to get kernel-only times
  --parse TRACE.csv PLAN.json   per-shape kernel time (sum of the op's launches, median over the calls) and GB/s of one-read-one-write bytes"""
import csv, json, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import oriented_object_detection_amd  # noqa
from oriented_object_detection_amd import ops

def timeit(fns, reps=30, inner=10):
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record(); b.synchronize()
            res[k].append(a.elapsed_time(b) * 1000 / inner)
    return [(statistics.median(r), min(r), max(r)) for r in res]

def fmt(t): return f"{t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"

if len(sys.argv) > 1 and sys.argv[1] == "--parse":
    rows = list(csv.DictReader(open(sys.argv[2])))
    name = next(k for k in rows[0] if k.lower() in ("kernel_name", "name"))
    t0 = next(k for k in rows[0] if k.lower() in ("start_timestamp", "start"))
    t1 = next(k for k in rows[0] if k.lower() in ("end_timestamp", "end"))
    mine = sorted(((int(r[t0]), int(r[t1]) - int(r[t0])) for r in rows if any(m in r[name] for m in ("k_headconv", "k_stemconv", "k_narrow_final"))))
    i = 0
    for label, per_call, calls, nbytes in json.load(open(sys.argv[3])):
        d = [sum(x[1] for x in mine[i + c * per_call:i + (c + 1) * per_call]) / 1e3 for c in range(calls)]
        i += per_call * calls
        print(f"{label}: kernel time {statistics.median(d):7.1f} us (min {min(d):.1f}, max {max(d):.1f}) = {nbytes / statistics.median(d) / 1e3:.0f} GB/s")
    assert i == len(mine), (i, len(mine))
    sys.exit(0)
KERNELS = len(sys.argv) > 1 and sys.argv[1] == "--kernels"
PLAN = []


def only_new(label, f, per_call, nbytes, calls=20):
    for _ in range(calls):
        f()
    torch.cuda.synchronize()
    PLAN.append((label, per_call, calls, nbytes))


B = 16
print("== head outputs, batch 16: new kernel vs zero-padded dense route; the same padded route twice gives its run-to-run spread")
for (H, cin, cout) in [(52, 64, 12), (26, 64, 12), (13, 64, 12), (52, 16, 1), (26, 16, 1), (13, 16, 1), (52, 128, 12), (26, 128, 12), (13, 128, 12), (52, 32, 1), (26, 32, 1), (13, 32, 1)]:
    W = H; N = B * H * W
    x = torch.randn(B, H, W, cin, device="cuda").to(torch.bfloat16)
    w = torch.randn(cout, cin, 1, 1, device="cuda") * 0.1
    b = torch.randn(cout, device="cuda")
    dy = torch.randn(B, H, W, cout, device="cuda")
    cp = (cout + 7) // 8 * 8
    dw, db = torch.empty_like(w), torch.empty_like(b)
    def new_f(): return ops.headconv_fwd_bf16(x, w, b)
    def new_b(): return ops.headconv_bwd_bf16(x, dy, w, dw_out=dw, db_out=db)
    wp = torch.zeros(cp, cin, 1, 1, device="cuda"); wp[:cout] = w  # resident: the padded rows live in the optimiser's buffers
    bp = torch.zeros(cp, device="cuda"); bp[:cout] = b
    def pad_f():
        return ops.conv_fwd_bf16(x, ops.conv_pack_bf16(wp, H, W), bp, cp, 1)[..., :cout].float()
    def pad_b():
        dp = torch.zeros(B, H, W, cp, device="cuda", dtype=torch.bfloat16); dp[..., :cout] = dy
        dwp = ops.conv_wgrad_c8_bf16(x, dp, 1)
        dbp = torch.empty(cp, device="cuda"); ops.bias_grad_bf16(dp, dbp)
        dx = ops.conv_fwd_bf16(dp, ops.conv_pack_bf16(wp, H, W, dgrad_form=True), None, cin, 1)
        return dx, dwp[:cout], dbp[:cout]
    bf = N * (cin * 2 + cout * 4) + cout * cin * 4
    bb = N * (cin * 2 + cout * 4 + cin * 2) + 2 * cout * cin * 4
    if KERNELS:
        only_new(f"{H}x{H} {cin}->{cout} fwd", new_f, 1, bf); only_new(f"{H}x{H} {cin}->{cout} bwd", new_b, 2, bb)
        continue
    tf = timeit([new_f, pad_f, pad_f]); tb = timeit([new_b, pad_b, pad_b])
    print(f"{H}x{H} {cin}->{cout}: fwd new {fmt(tf[0])} = {bf / tf[0][0] / 1e3:.0f} GB/s | padded {fmt(tf[1])} / {fmt(tf[2])}")
    print(f"{H}x{H} {cin}->{cout}: bwd new {fmt(tb[0])} = {bb / tb[0][0] / 1e3:.0f} GB/s | padded {fmt(tb[1])} / {fmt(tb[2])}")
    sys.stdout.flush()

print("== stem 416 x 416, batch 16")
for cin, cout in [(3, 16), (3, 32)]:
    H = W = 416
    x = torch.randint(0, 256, (B, H, W, cin), device="cuda", dtype=torch.uint8)
    w = torch.randn(cout, cin, 3, 3, device="cuda") * 0.2
    dz = torch.randn(B, H // 2, W // 2, cout, device="cuda").to(torch.bfloat16)
    dw = torch.empty_like(w)
    def new_f(): return ops.stemconv_fwd_u8(x, w)
    def new_w(): return ops.stemconv_wgrad_u8(x, dz, out=dw)
    def padx():
        xp = torch.zeros(B, H, W, 8, device="cuda", dtype=torch.bfloat16); xp[..., :cin] = (x.float() / 255.0).to(torch.bfloat16)
        return xp
    wp = torch.zeros(cout, 8, 3, 3, device="cuda"); wp[:, :cin] = w
    def pad_f():
        return ops.conv_fwd_bf16(padx(), ops.conv_pack_bf16(wp, H, W, stride=2), None, cout, 3, stride=2)
    def pad_w():
        return ops.conv_wgrad_c8_bf16(padx(), dz, 3, stride=2)[:, :cin]
    bf = B * H * W * cin + B * (H // 2) * (W // 2) * cout * 2
    if KERNELS:
        only_new(f"stem {cin}->{cout} fwd", new_f, 1, bf); only_new(f"stem {cin}->{cout} wgrad", new_w, 2, bf)
        continue
    tf = timeit([new_f, pad_f, pad_f], reps=15, inner=4); tw = timeit([new_w, pad_w, pad_w], reps=15, inner=4)
    print(f"stem {cin}->{cout}: fwd new {fmt(tf[0])} = {bf / tf[0][0] / 1e3:.0f} GB/s | padded {fmt(tf[1])} / {fmt(tf[2])}")
    print(f"stem {cin}->{cout}: wgrad new {fmt(tw[0])} = {bf / tw[0][0] / 1e3:.0f} GB/s | padded {fmt(tw[1])} / {fmt(tw[2])}")
    sys.stdout.flush()
if KERNELS:
    json.dump(PLAN, open(sys.argv[2], "w"))
