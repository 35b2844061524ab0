"""CPU references (plain torch, fp64, NHWC) for the depthwise 3x3 kernels of csrc/dwgrad.hip and the BatchNorm with an optional activation of
csrc/bntrain.hip -- not the product, nothing here touches the GPU.  Shared by test_train_dw_cpu.py (which pins them against torch.autograd) and
test_gpu_train_dw.py.

  dw_fwd_ref(x, w)            z[b,i,j,c] = sum_{ky,kx} w[c,0,ky,kx] x[b, i+ky-1, j+kx-1, c]   (x [B,H,W,C], w [C,1,3,3], zero padding)
  dw_bwd_ref(x, dz, w)        -> (dx, dw): dx[b,i,j,c] = sum w[c,0,ky,kx] dz[b, i-ky+1, j-kx+1, c];  dw[c,0,ky,kx] = sum dz[b,i,j,c] x[b, i+ky-1, j+kx-1, c]
  bn_ref(z, gamma, beta, eps, act)   training-mode BatchNorm over the rows of z [..., C] (biased batch variance), SiLU when act
  bf16(t)                     t rounded to bf16 (nearest even), in t's dtype

and the nn-module reference of the assembled tests (fp64, NCHW, torch.autograd), evaluated PLAIN (no rounding anywhere) or ROUNDED to bf16 at the
device's rounding points (x, the weights, z, a, da, dz, dx):

  dwbn_case / pair_case       the seeded cases;  run_dwbn / run_pair(case, rounded) -> {name: tensor};  rel_dist(a, b)"""
import torch
import torch.nn as nn
import torch.nn.functional as F

EPS, MOM = 1e-3, 0.03  # Ultralytics' initialize_weights values

# (B, H, W, C) of the per-element GPU tests (test_gpu_train_dw.py) and of the geometry checks (test_train_dw_cpu.py)
CATALOGUE = [(2, 52, 52, 64), (2, 26, 26, 128), (2, 26, 26, 64), (2, 13, 13, 256), (2, 13, 13, 64), (2, 13, 13, 128),  # yolo11n at 416 px
             (1, 52, 52, 128), (2, 26, 26, 256), (2, 13, 13, 512),                                                     # yolo11s
             (2, 16, 16, 64), (2, 8, 8, 128), (3, 4, 4, 256)]                                                          # the 128-px maps
EDGES = [(2, 13, 9, 64), (2, 9, 13, 64), (2, 52, 36, 64), (1, 1, 1, 8), (2, 2, 1, 8), (2, 1, 2, 8), (1, 3, 7, 24), (5, 6, 6, 264), (1, 26, 26, 64)]
# One shape on each side of every branch of the launcher (dw_geo in csrc/dwgrad.hip):
#   stripe height R = 2 up to 16 rows, 4 above     (2,16,16,64) above | (1,17,3,8) here: the first map with R = 4, and a last stripe of 1 row
#   last stripe full or short                      52 = 13 x 4 and 16 = 8 x 2 full | 13, 9, 3, 1 (R = 2) and 26, 17 (R = 4) short; (1,1,1,8): H < R
#   slab count 1 or more                           (1,1,1,8), (2,2,1,8), (2,1,2,8), (1,3,7,24): one workgroup | every other shape: several
#   lane run of 1 run or 2 (more than 512 slabs' worth of runs)   every shape above: 1 | (2,16,260,256) here: 4160 runs on 512 x 8 lanes, the second
#                                                  pass only partly filled
#   column groups 1 or 2 (more than 32 chunks)     (5,6,6,264) above: 33 chunks | every other shape: 1
#   lanes per chunk not a power of two             (1,3,7,24) above: 3 chunk columns x 85 rows, one thread idle
BRANCHES = [(1, 17, 3, 8), (2, 16, 260, 256)]
DW_SHAPES = CATALOGUE + EDGES + BRANCHES


def bf16(t):
    return t.float().to(torch.bfloat16).to(t.dtype)


def _pad(t):
    return F.pad(t, (0, 0, 1, 1, 1, 1))  # [B,H+2,W+2,C]


def dw_fwd_ref(x, w):
    B, H, W, C = x.shape
    p, z = _pad(x), torch.zeros_like(x)
    for ky in range(3):
        for kx in range(3):
            z = z + w[:, 0, ky, kx] * p[:, ky:ky + H, kx:kx + W]
    return z


def dw_bwd_ref(x, dz, w):
    B, H, W, C = x.shape
    px, pz = _pad(x), _pad(dz)
    dx, dw = torch.zeros_like(x), torch.zeros_like(w)
    for ky in range(3):
        for kx in range(3):
            dx = dx + w[:, 0, ky, kx] * pz[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]
            dw[:, 0, ky, kx] = (dz * px[:, ky:ky + H, kx:kx + W]).sum(dim=(0, 1, 2))
    return dx, dw


def bn_ref(z, gamma, beta, eps, act):
    C = z.shape[-1]
    r = z.reshape(-1, C)
    y = gamma * (r - r.mean(0)) / torch.sqrt(r.var(0, unbiased=False) + eps) + beta
    return (F.silu(y) if act else y).reshape(z.shape)


# ---------------------------------------------------------------------------------------------- the assembled reference
def _q(t):
    """bf16 rounding point with a straight-through gradient."""
    return t + (bf16(t) - t).detach()


class _GradBf16(torch.autograd.Function):
    """identity forward; the gradient is rounded to bf16 on its way back (a gradient tensor the device stores in bf16)"""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


class RefBlock:
    """nn.Sequential(Conv2d(c1, c2, k, 1, k // 2, groups=g, bias=False), BatchNorm2d(c2, eps=1e-3, momentum=0.03)[, SiLU]) in .train(), fp64."""

    def __init__(self, g, c1, c2, k, groups, act):
        mods = [nn.Conv2d(c1, c2, k, 1, k // 2, groups=groups, bias=False), nn.BatchNorm2d(c2, eps=EPS, momentum=MOM)] + ([nn.SiLU()] if act else [])
        self.seq = nn.Sequential(*mods).train()
        self.groups, self.k, self.act = groups, k, act
        fan = c1 // groups * k * k
        with torch.no_grad():
            self.seq[0].weight.copy_(torch.randn(c2, c1 // groups, k, k, generator=g) * (1.5 / fan ** 0.5))
            self.seq[1].weight.copy_(torch.rand(c2, generator=g) + 0.5)
            self.seq[1].bias.copy_(torch.randn(c2, generator=g) * 0.2)
            self.seq[1].running_mean.copy_(torch.randn(c2, generator=g) * 0.1)
            self.seq[1].running_var.copy_(torch.rand(c2, generator=g) + 0.5)
        self.init = tuple(t.detach().clone() for t in (self.seq[0].weight, self.seq[1].weight, self.seq[1].bias, self.seq[1].running_mean, self.seq[1].running_var))
        self.seq.double()

    def reset(self):
        """back to the initial parameters and running statistics, gradients cleared (every evaluation starts from the same state)"""
        with torch.no_grad():
            for dst, src in zip((self.seq[0].weight, self.seq[1].weight, self.seq[1].bias, self.seq[1].running_mean, self.seq[1].running_var), self.init):
                dst.copy_(src)
        for p in self.seq.parameters():
            p.grad = None

    def _conv(self, x, w):
        """The Conv2d of the stack.  A depthwise one is evaluated as nine shifted products: torch's fp64 grouped convolution takes seconds per
        call on the CPU, and test_train_dw_cpu.py pins the two to 1e-12 of each other."""
        if self.groups == 1:
            return F.conv2d(x, w, padding=self.k // 2)
        H, W = x.shape[2], x.shape[3]
        p = F.pad(x, (1, 1, 1, 1))
        return sum(w[:, 0, ky, kx].view(1, -1, 1, 1) * p[:, :, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3))

    def __call__(self, x, rounded):
        conv, tail = self.seq[0], self.seq[1:]
        if not rounded:
            return tail(self._conv(x, conv.weight))  # the module stack itself
        x = _GradBf16.apply(x)                                      # dx
        z = _GradBf16.apply(_q(self._conv(x, _q(conv.weight))))     # the weights, z; dz
        return _GradBf16.apply(_q(tail(z)))                         # a, da

    def results(self, tag):
        conv, bn = self.seq[0], self.seq[1]
        return {f"{tag}dW": conv.weight.grad.clone(), f"{tag}dgamma": bn.weight.grad.clone(), f"{tag}dbeta": bn.bias.grad.clone(),
                f"{tag}rmean": bn.running_mean.clone(), f"{tag}rvar": bn.running_var.clone()}


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _grad_in(g, *shape):
    """The incoming gradient of a case: N(0, 0.1^2) on the grid of 2^-7.  Such values are bf16, and their fp32 sums are exact in any order, so a
    quantity that no rounding point touches (dbeta of a block without activation is the plain sum of da) has e = 0 and the device can meet it."""
    return (torch.round(torch.randn(*shape, generator=g) * 12.8) / 128).to(torch.bfloat16)


def dwbn_case(B, H, W, C, act):
    """-> (block, x bf16 NHWC, da bf16 NHWC): the seeded case of the DWConvBN tests."""
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C + int(act))
    blk = RefBlock(g, C, C, 3, C, act)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    da = _grad_in(g, B, H, W, C)
    return blk, x, da


def pair_case(B, H, W, c1, c2):
    """-> (dw block, pw block, x, da): DWConv 3x3 -> Conv 1x1, both with BatchNorm and SiLU (one pair of Detect.cv3[i])."""
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + c1 + c2)
    dw, pw = RefBlock(g, c1, c1, 3, c1, True), RefBlock(g, c1, c2, 1, 1, True)
    x = torch.randn(B, H, W, c1, generator=g).to(torch.bfloat16)
    da = _grad_in(g, B, H, W, c2)
    return dw, pw, x, da


def _run(blocks, tags, x, da, rounded):
    for b in blocks:
        b.reset()
    xr = _nchw(x).clone().requires_grad_(True)
    a = xr
    for b in blocks:
        a = b(a, rounded)
    a.backward(_nchw(da))
    out = {"out": a.detach().clone(), "dx": xr.grad.clone()}
    for b, t in zip(blocks, tags):
        out.update(b.results(t))
    return out


def run_dwbn(case, rounded):
    blk, x, da = case
    return _run([blk], [""], x, da, rounded)


def run_pair(case, rounded):
    dw, pw, x, da = case
    return _run([dw, pw], ["dw.", "pw."], x, da, rounded)


def rel_dist(a, b):
    """max |a - b| / max |b|"""
    return float((a.double() - b.double()).abs().max()) / float(b.double().abs().max())
