"""CPU references (plain torch, fp64, NHWC) for the gradient-routing kernels of csrc/routegrad.hip -- not the product, nothing here touches the
GPU.  Shared by test_train_route_cpu.py (which pins them against torch.autograd) and test_gpu_train_route.py.

  pools_ref(x)               [B,H,W,C] -> cat [B,H,W,4C] = [x, y1, y2, y3], y_k = maxpool5x5(y_{k-1}) (stride 1, pad 2, -inf padding)
  pools_bwd_ref(cat, dcat)   -> dx [B,H,W,C]; the argmax of level k is recomputed from member k - 1 of cat as the FIRST maximum in a row-major
                             scan of the window (strict `>` while scanning dy then dx): what torch's max_pool2d does
  upcat_ref(a, b, up)        cat(nearest_upsample(a), b) along C
  upcat_bwd_ref(dout, Ca, up, da0=None, db0=None) -> (da, db); da0 / db0: prior values added (the accumulate form)

and the nn-module reference of the block tests (fp32, NCHW, torch.autograd):

  RefConvBN                  Conv2d(bias=False) -> BatchNorm2d(eps 1e-3, momentum 0.03).train() -> SiLU at the device's bf16 rounding points
  ref_sppf(cv1, cv2, x, a1_pin=None, grad_bf16=False)   SPPF from two of them around F.max_pool2d"""
import torch
import torch.nn as nn
import torch.nn.functional as F

EPS, MOM = 1e-3, 0.03  # Ultralytics' initialize_weights values

K, R = 5, 2
NEG = float("-inf")


def _first_max(v):
    """v [B,H,W,C] -> (max over the 5x5 window, window offset 0..24 of its first maximum in dy-then-dx order), both [B,H,W,C]."""
    B, H, W, C = v.shape
    pad = torch.full((B, H + 2 * R, W + 2 * R, C), NEG, dtype=v.dtype)
    pad[:, R:R + H, R:R + W] = v
    m = torch.full_like(v, NEG)
    idx = torch.full(v.shape, -1, dtype=torch.int64)
    for dy in range(K):
        for dx in range(K):
            s = pad[:, dy:dy + H, dx:dx + W]
            upd = s > m
            m = torch.where(upd, s, m)
            idx = torch.where(upd, torch.full_like(idx, dy * K + dx), idx)
    return m, idx


def pools_ref(x):
    ys = [x]
    for _ in range(3):
        ys.append(_first_max(ys[-1])[0])
    return torch.cat(ys, dim=-1)


def pools_bwd_ref(cat, dcat):
    B, H, W, C4 = cat.shape
    C = C4 // 4
    g = dcat[..., 3 * C:].clone()
    for k in (3, 2, 1):
        _, idx = _first_max(cat[..., (k - 1) * C:k * C])
        acc = torch.zeros((B, H + 2 * R, W + 2 * R, C), dtype=dcat.dtype)
        for dy in range(K):
            for dx in range(K):
                # output q with its argmax at window offset (dy, dx) sends g[q] to input p = q + (dy - 2, dx - 2)
                acc[:, dy:dy + H, dx:dx + W] += torch.where(idx == dy * K + dx, g, torch.zeros_like(g))
        g = dcat[..., (k - 1) * C:k * C] + acc[:, R:R + H, R:R + W]
    return g


def upcat_ref(a, b, up):
    return torch.cat([a.repeat_interleave(up, dim=1).repeat_interleave(up, dim=2), b], dim=-1)


def upcat_bwd_ref(dout, Ca, up, da0=None, db0=None):
    B, uH, uW, _ = dout.shape
    H, W = uH // up, uW // up
    da = dout[..., :Ca].reshape(B, H, up, W, up, Ca).sum(dim=(2, 4))
    db = dout[..., Ca:].clone()
    if da0 is not None:
        da = da + da0
    if db0 is not None:
        db = db + db0
    return da, db


def q(t):
    """bf16 rounding point with a straight-through gradient."""
    return t + (t.to(torch.bfloat16).float() - t).detach()


class _GradBf16(torch.autograd.Function):
    """identity forward; the gradient is rounded to bf16 on its way back (a gradient tensor the device stores in bf16)"""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


class RefConvBN:
    """Conv2d(bias=False) -> BatchNorm2d(eps 1e-3, momentum 0.03) in .train() -> SiLU with the device's bf16 rounding points (weights, z, a).
    grad_bf16: also round the gradients the device stores in bf16 on the way back (dz, and dx of the conv); autograd alone rounds none."""

    def __init__(self, g, c1, c2, k=1, s=1):
        self.k, self.s = k, s
        self.w = nn.Parameter(torch.randn(c2, c1, k, k, generator=g) * (1.5 / (c1 * k * k) ** 0.5))
        self.bn = nn.BatchNorm2d(c2, eps=EPS, momentum=MOM).train()
        with torch.no_grad():
            self.bn.weight.copy_(torch.rand(c2, generator=g) + 0.5)
            self.bn.bias.copy_(torch.randn(c2, generator=g) * 0.2)
            self.bn.running_mean.copy_(torch.randn(c2, generator=g) * 0.1)
            self.bn.running_var.copy_(torch.rand(c2, generator=g) + 0.5)

    def device_args(self):
        """(w, gamma, beta, running_mean, running_var) on the device, BEFORE the reference's forward updates the running statistics."""
        return tuple(t.detach().clone().cuda() for t in (self.w, self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var))

    def __call__(self, x, grad_bf16=False):
        if grad_bf16:
            x = _GradBf16.apply(x)   # the conv's dx
        z = q(F.conv2d(x, q(self.w), stride=self.s, padding=self.k // 2))
        if grad_bf16:
            z = _GradBf16.apply(z)   # the BatchNorm backward's dz
        return q(F.silu(self.bn(z)))

    def params(self):
        return [self.w, self.bn.weight, self.bn.bias]


def ref_sppf(cv1, cv2, xr, a1_pin=None, grad_bf16=False):
    """-> (a1_ref, out_ref).  a1_pin: the pools' input is pinned to these values (the device's bf16 a1) by straight-through substitution -- one
    flipped bf16 rounding of a1 would move an argmax and with it a whole gradient; a1 itself is compared on its own.  grad_bf16: round every gradient tensor
    the device stores in bf16 on the way back: cv2's dz, dcat, the pools' dx, cv1's dz and dx."""
    a1 = cv1(xr, grad_bf16)
    a1p = a1 if a1_pin is None else a1 + (a1_pin - a1).detach()
    if grad_bf16:
        a1p = _GradBf16.apply(a1p)   # the pools' dx
    ys = [a1p]
    for _ in range(3):
        ys.append(F.max_pool2d(ys[-1], 5, 1, 2))
    return a1, cv2(torch.cat(ys, dim=1), grad_bf16)   # (cv2's own input rounding is dcat)


def sppf_case(B, H, W, c1, c2):
    """The seeded case of the SPPF block tests -> (cv1, cv2, x bf16 NHWC, da bf16 NHWC)."""
    g = torch.Generator().manual_seed(B * 100 + H + c1)
    cv1, cv2 = RefConvBN(g, c1, c1 // 2), RefConvBN(g, 2 * c1, c2)
    x = torch.randn(B, H, W, c1, generator=g).to(torch.bfloat16)
    da = (torch.randn(B, H, W, c2, generator=g) * 0.1).to(torch.bfloat16)
    return cv1, cv2, x, da


# ---------------------------------------------------------------------------------------------- the block tests' bounds
BF, U = 2.0 ** -8, 2.0 ** -24
# A figure of (nearly) zero gives no bound by itself: the bound is then the reference's own grain -- one flipped bf16 rounding of the largest element
# for the bf16 tensors, the fp32 reference's summation error (16 roundings of 2^-24) for the fp32 gradients and statistics.
FLOOR = {"out": BF, "dx": BF, "dskip": BF, "dW": 16 * U, "dgamma": 16 * U, "dbeta": 16 * U, "rmean": 16 * U, "rvar": 16 * U,
         "db": 16 * U}  # (db: the bias gradient of the head's plain output convs, a per-channel sum of the incoming gradient like dbeta)
# measured (MI355X), max |d| / max |ref| of every compared quantity, per SPPF case (B, H, W, c1, c2); asserted at 2.5 x its own figure
SPPF_MEASURED = {
    (2, 13, 13, 256, 256): {"out": 3.09e-3, "dx": 6.87e-3, "cv1.dW": 5.91e-3, "cv1.dgamma": 1.09e-2, "cv1.dbeta": 1.54e-2, "cv1.rmean": 6.89e-7,
                            "cv1.rvar": 7.81e-8, "cv2.dW": 4.84e-3, "cv2.dgamma": 1.80e-5, "cv2.dbeta": 1.35e-5, "cv2.rmean": 3.48e-6, "cv2.rvar": 1.62e-7},
    (2, 4, 4, 128, 128): {"out": 0.0, "dx": 4.96e-3, "cv1.dW": 4.01e-3, "cv1.dgamma": 1.01e-2, "cv1.dbeta": 1.28e-2, "cv1.rmean": 0.0, "cv1.rvar": 8.29e-8,
                          "cv2.dW": 4.46e-3, "cv2.dgamma": 1.21e-7, "cv2.dbeta": 1.61e-7, "cv2.rmean": 0.0, "cv2.rvar": 0.0}}
