"""CPU references (plain torch, fp64, NHWC) for the narrow-channel kernels of csrc/narrowgrad.hip -- the head's 1x1 + bias outputs and the stem on the
uint8 tile -- not the product, nothing here touches the GPU.  Shared by test_train_narrow_cpu.py (which pins them against torch.autograd) and
test_gpu_train_narrow.py.  The per-element references take the bf16-ROUNDED weights (and, for the head's backward, the bf16-rounded dy).

  head_fwd_ref(x, w, b)        y[n,o] = sum_c w[o,c] x[n,c] + b[o]                     x [..., cin], w [cout,cin], b [cout] or None
  head_bwd_ref(x, dy, w)       -> (dx, dw, db): dx = dy w;  dw[o,c] = sum_n dy[n,o] x[n,c];  db[o] = sum_n dy[n,o]
  stem_operand(x_u8)           bf16(v / 255) as fp64 (an fp32 division, then nearest even)
  stem_fwd_ref(xq, w)          z[b,i,j,o] = sum w[o,c,ky,kx] xq[b, 2i+ky-1, 2j+kx-1, c]      xq [B,H,W,cin], w [cout,cin,3,3], zero padding
  stem_wgrad_ref(xq, dz)       dw[o,c,ky,kx] = sum dz[b,i,j,o] xq[b, 2i+ky-1, 2j+kx-1, c]

and the nn-module references of the assembled tests (fp64, NCHW, torch.autograd), evaluated PLAIN or ROUNDED to bf16 at the device's rounding
points, in the scheme of dw_ref.py:  stem_case / head_case / angle_case / class_case;  run_*(case, rounded) -> {name: tensor}."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from dw_ref import EPS, MOM, RefBlock, _GradBf16, _q, bf16, rel_dist  # noqa: F401

# (B, H, W, cin, cout) of the per-element GPU tests
HEAD_SHAPES = [(1, 1, 1, 8, 1), (2, 7, 5, 16, 1), (2, 7, 5, 64, 3), (2, 13, 13, 64, 12), (3, 13, 9, 128, 12), (2, 26, 18, 64, 16), (1, 13, 13, 256, 17),
               (2, 5, 3, 512, 64), (2, 52, 52, 16, 1)]
STEM_SHAPES = [(1, 1, 1, 3, 8), (2, 2, 1, 4, 16), (2, 7, 5, 3, 16), (3, 16, 16, 4, 32), (2, 27, 13, 3, 32), (2, 52, 36, 3, 16), (1, 64, 64, 4, 64),
               (1, 416, 416, 3, 16)]

# The tolerances of the assembled GPU tests: e = max |rounded - plain| / max |plain| per tensor, MEASURED by test_train_narrow_cpu.py (which keeps
# each figure in the band [1 / 1.5, 1.5] x the value recorded here); test_gpu_train_narrow.py recomputes e from the same functions and requires the
# device within 2 e of plain (dw_ref.py / test_train_dw_cpu.py's scheme and margin).
E_STEM = {"out": 4.82e-03, "dW": 3.31e-03, "dgamma": 2.41e-03, "dbeta": 1.88e-03, "rmean": 5.97e-04, "rvar": 1.59e-05}
E_HEAD = {"out": 1.62e-03, "dx": 5.08e-03, "dW": 1.50e-03, "db": 1.34e-03}
# the angle branch's incoming gradient is on the grid of 2^-7: bf16 values with exact fp32 sums, so out.db (their plain sum) has e = 0 and the
# device has to be exact (dw_ref._grad_in)
E_ANGLE = {"out": 5.58e-03, "dx": 6.94e-03, "c0.dW": 6.19e-03, "c0.dgamma": 5.25e-03, "c0.dbeta": 5.49e-03, "c0.rmean": 5.79e-05, "c0.rvar": 4.77e-05,
           "c1.dW": 5.20e-03, "c1.dgamma": 4.27e-03, "c1.dbeta": 2.94e-03, "c1.rmean": 3.42e-04, "c1.rvar": 2.58e-05, "out.dW": 4.79e-03, "out.db": 0.0}
E_CLASS = {"loss": 3.96e-05, "dx": 1.69e-02, "p0.dw.dW": 1.27e-02, "p0.dw.dgamma": 1.69e-02, "p0.dw.dbeta": 1.45e-02, "p0.dw.rmean": 9.89e-05,
           "p0.dw.rvar": 2.43e-04, "p0.pw.dW": 1.12e-02, "p0.pw.dgamma": 1.73e-02, "p0.pw.dbeta": 1.04e-02, "p0.pw.rmean": 1.59e-04, "p0.pw.rvar": 3.30e-05,
           "p1.dw.dW": 8.64e-03, "p1.dw.dgamma": 6.49e-03, "p1.dw.dbeta": 8.19e-03, "p1.dw.rmean": 3.37e-04, "p1.dw.rvar": 1.14e-04, "p1.pw.dW": 6.70e-03,
           "p1.pw.dgamma": 1.61e-03, "p1.pw.dbeta": 1.41e-03, "p1.pw.rmean": 1.26e-04, "p1.pw.rvar": 9.81e-05, "out.dW": 1.59e-03, "out.db": 4.33e-04}


def head_fwd_ref(x, w, b=None):
    y = x @ w.t()
    return y if b is None else y + b


def head_bwd_ref(x, dy, w):
    cin, cout = x.shape[-1], dy.shape[-1]
    x2, d2 = x.reshape(-1, cin), dy.reshape(-1, cout)
    return (d2 @ w).reshape(x.shape), d2.t() @ x2, d2.sum(0)


def stem_operand(x_u8):
    return (x_u8.float() / 255.0).to(torch.bfloat16).double()


def _taps(xq, Ho, Wo):
    """yields (ky, kx, window [B,Ho,Wo,cin]) of the stride-2, pad-1 3x3 conv"""
    p = F.pad(xq, (0, 0, 1, 2, 1, 2))
    for ky in range(3):
        for kx in range(3):
            yield ky, kx, p[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]


def stem_fwd_ref(xq, w):
    B, H, W, _ = xq.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    z = torch.zeros(B, Ho, Wo, w.shape[0], dtype=xq.dtype)
    for ky, kx, win in _taps(xq, Ho, Wo):
        z = z + win @ w[:, :, ky, kx].t()
    return z


def stem_wgrad_ref(xq, dz):
    B, H, W, cin = xq.shape
    Ho, Wo, cout = dz.shape[1], dz.shape[2], dz.shape[3]
    dw = torch.zeros(cout, cin, 3, 3, dtype=xq.dtype)
    for ky, kx, win in _taps(xq, Ho, Wo):
        dw[:, :, ky, kx] = dz.reshape(-1, cout).t() @ win.reshape(-1, cin)
    return dw


# ---------------------------------------------------------------------------------------------- the assembled references
def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _grad_in(g, *shape):
    return (torch.round(torch.randn(*shape, generator=g) * 12.8) / 128).to(torch.bfloat16)


class RefStem:
    """nn.Sequential(Conv2d(cin, c2, 3, 2, 1, bias=False), BatchNorm2d(c2, eps=1e-3, momentum=0.03), SiLU) in .train(), fp64, on v / 255."""

    def __init__(self, g, cin, c2):
        self.seq = nn.Sequential(nn.Conv2d(cin, c2, 3, 2, 1, bias=False), nn.BatchNorm2d(c2, eps=EPS, momentum=MOM), nn.SiLU()).train()
        with torch.no_grad():
            self.seq[0].weight.copy_(torch.randn(c2, cin, 3, 3, generator=g) * (1.5 / (cin * 9) ** 0.5))
            self.seq[1].weight.copy_(torch.rand(c2, generator=g) + 0.5)
            self.seq[1].bias.copy_(torch.randn(c2, generator=g) * 0.2)
            self.seq[1].running_mean.copy_(torch.randn(c2, generator=g) * 0.1)
            self.seq[1].running_var.copy_(torch.rand(c2, generator=g) + 0.5)
        self.init = tuple(t.detach().clone() for t in (self.seq[0].weight, self.seq[1].weight, self.seq[1].bias, self.seq[1].running_mean, self.seq[1].running_var))
        self.seq.double()

    reset = RefBlock.reset
    results = RefBlock.results

    def __call__(self, x_u8, rounded):
        conv, tail = self.seq[0], self.seq[1:]
        if not rounded:
            return self.seq(_nchw(x_u8) / 255.0)
        z = _GradBf16.apply(_q(F.conv2d(_nchw(stem_operand(x_u8)), _q(conv.weight), stride=2, padding=1)))  # the operand, the weights, z; dz
        return _GradBf16.apply(_q(tail(z)))                                                                 # a, da


class RefHead:
    """nn.Conv2d(c, cout, 1) with bias, fp64.  Rounded: the weights to bf16, the logits NOT (fp32 on the device), the incoming gradient and dx to bf16."""

    def __init__(self, g, c, cout):
        self.conv = nn.Conv2d(c, cout, 1)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(cout, c, 1, 1, generator=g) * (1.5 / c ** 0.5))
            self.conv.bias.copy_(torch.randn(cout, generator=g) * 0.5)
        self.init = (self.conv.weight.detach().clone(), self.conv.bias.detach().clone())
        self.conv.double()

    def reset(self):
        with torch.no_grad():
            self.conv.weight.copy_(self.init[0]); self.conv.bias.copy_(self.init[1])
        self.conv.weight.grad = self.conv.bias.grad = None

    def __call__(self, x, rounded):
        if not rounded:
            return self.conv(x)
        return _GradBf16.apply(F.conv2d(_GradBf16.apply(x), _q(self.conv.weight), self.conv.bias))  # dx; the weights; dy

    def results(self, tag):
        return {f"{tag}dW": self.conv.weight.grad.clone(), f"{tag}db": self.conv.bias.grad.clone()}


def stem_case(B=2, H=52, W=36, cin=3, c2=16):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + cin + c2)
    blk = RefStem(g, cin, c2)
    x = torch.randint(0, 256, (B, H, W, cin), generator=g, dtype=torch.uint8)
    return blk, x, _grad_in(g, B, (H + 1) // 2, (W + 1) // 2, c2)


def run_stem(case, rounded):
    blk, x, da = case
    blk.reset()
    a = blk(x, rounded)
    a.backward(_nchw(da))
    return {"out": a.detach().clone(), **blk.results("")}


def head_case(B=2, H=13, W=13, c=64, cout=12):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + c + cout)
    head = RefHead(g, c, cout)
    x = torch.randn(B, H, W, c, generator=g).to(torch.bfloat16)
    dy = torch.randn(B, H, W, cout, generator=g) * 0.1  # fp32, NOT bf16 values: the kernel rounds them
    return head, x, dy


def run_head(case, rounded):
    head, x, dy = case
    head.reset()
    xr = _nchw(x).clone().requires_grad_(True)
    y = head(xr, rounded)
    y.backward(_nchw(dy))
    return {"out": y.detach().clone(), "dx": xr.grad.clone(), **head.results("")}


def angle_case(B=2, H=13, W=13, c=64, c4=16):
    """ConvBN 3x3 (c -> c4) -> ConvBN 3x3 (c4 -> c4) -> Conv2d 1x1 (c4 -> 1): OBB.cv4[i] of yolo11n.  The incoming gradient is on the grid of 2^-7."""
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + c + c4)
    blocks = [RefBlock(g, c, c4, 3, 1, True), RefBlock(g, c4, c4, 3, 1, True)]
    head = RefHead(g, c4, 1)
    x = torch.randn(B, H, W, c, generator=g).to(torch.bfloat16)
    return blocks, head, x, _grad_in(g, B, H, W, 1).float()


def run_angle(case, rounded):
    blocks, head, x, dy = case
    for b in blocks + [head]:
        b.reset()
    xr = _nchw(x).clone().requires_grad_(True)
    a = xr
    for b in blocks:
        a = b(a, rounded)
    y = head(a, rounded)
    y.backward(_nchw(dy))
    out = {"out": y.detach().clone(), "dx": xr.grad.clone()}
    for i, b in enumerate(blocks):
        out.update(b.results(f"c{i}."))
    out.update(head.results("out."))
    return out


def class_case(B=2, H=13, W=13, c=64, c3=64, nc=12):
    """Detect.cv3[i]: (DWConv 3x3 -> Conv 1x1) x 2 -> Conv2d 1x1 (c3 -> nc) under BCEWithLogits(sum) / target_scores_sum."""
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + c + c3 + nc)
    pairs = [(RefBlock(g, c, c, 3, c, True), RefBlock(g, c, c3, 1, 1, True)), (RefBlock(g, c3, c3, 3, c3, True), RefBlock(g, c3, c3, 1, 1, True))]
    head = RefHead(g, c3, nc)
    x = torch.randn(B, H, W, c, generator=g).to(torch.bfloat16)
    t = torch.rand(B, H, W, nc, generator=g) * (torch.rand(B, H, W, nc, generator=g) < 0.1).float()  # sparse soft targets
    return pairs, head, x, t, max(float(t.sum()), 1.0)


def run_class(case, rounded):
    pairs, head, x, t, tss = case
    blocks = [b for p in pairs for b in p]
    for b in blocks + [head]:
        b.reset()
    xr = _nchw(x).clone().requires_grad_(True)
    a = xr
    for b in blocks:
        a = b(a, rounded)
    y = head(a, rounded)
    loss = F.binary_cross_entropy_with_logits(y, _nchw(t), reduction="sum") / tss
    loss.backward()
    out = {"loss": loss.detach().reshape(1).clone(), "dx": xr.grad.clone()}
    for i, (dw, pw) in enumerate(pairs):
        out.update(dw.results(f"p{i}.dw."))
        out.update(pw.results(f"p{i}.pw."))
    out.update(head.results("out."))
    return out
