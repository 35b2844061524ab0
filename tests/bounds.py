"""Helpers shared by the per-element GPU tests (test_gpu_train_shapes.py, test_gpu_train_loss.py) and the CPU checks of the
conditioning floor (test_train_loss_cpu.py).  Plain module, no fixtures: nothing here touches the GPU until a Guarded buffer is built.

  Guarded        an output buffer between two 4 KiB guard bands, every byte 0xff (a NaN in bf16 and fp32)
  _check         |got - ref| <= bound element-wise, printing the worst |err| / bound
  _same_thrice   bit-identical results before and after a larger call grows a workspace slot
  spread         the conditioning floor: the spread of an fp64 formula over K random relative perturbations of up to 16 u of every input
                 (and, where the formula takes a `rnd` hook, of every intermediate: Monte Carlo arithmetic, Parker 1997)"""
import math

import torch

U = 2.0 ** -24  # fp32 unit roundoff
GUARD = 4096


class Guarded:
    """[4 KiB guard | output (16-byte aligned) | 4 KiB guard] in one device allocation, every byte 0xff; `init` fills the output part."""

    def __init__(self, shape, dtype, init=None):
        n = math.prod(shape)
        self.nb = n * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((GUARD + self.nb + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.out = self.raw[GUARD:GUARD + self.nb].view(dtype).view(shape)
        if init is not None:
            self.out.copy_(init)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xFF).all()) and bool((self.raw[GUARD + self.nb:] == 0xFF).all())

    def get(self, what):
        torch.cuda.synchronize()
        assert self.guards_intact(), f"{what}: write outside the output"
        assert bool(torch.isfinite(self.out.float()).all()), f"{what}: output element not written (NaN fill left) or not finite"
        return self.out.clone()


def _check(what, got, ref, bound):
    """|got - ref| <= bound element-wise (fp64); prints the worst ratio (the margin)."""
    got = got.double().cpu().reshape(ref.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    d = (got - ref).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"  {what}: max |got - ref| / bound = {worst:.3f}")
    if not worst <= 1:
        i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
        raise AssertionError(f"{what}: element {i} (of shape {tuple(ref.shape)}) got {float(got.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, "
                             f"bound {float(bound.flatten()[i]):.3e}")


def _same_thrice(what, run, grow):
    """run() -> tensor; grow() runs the op at a larger shape (its workspace slot grows); the first and the third result are bit-identical."""
    a = run().clone()
    grow()
    b = run()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a, b.view(torch.uint8) if b.dtype != torch.uint8 else b), \
        f"{what}: not bit-identical after the workspace grew"


class _Rounding(torch.autograd.Function):
    """t (1 + d) forward; the incoming gradient times (1 + d) (1 + d'') backward: the rounding of the backward's own operations"""

    @staticmethod
    def forward(ctx, t, a, b):
        ctx.save_for_backward(a * b)
        return t * a

    @staticmethod
    def backward(ctx, g):
        (ab,) = ctx.saved_tensors
        return g * ab, None, None


def spread(f, inputs, k=8, rel=16 * U, seed=0, rel_mid=None):
    """f(*inputs, rnd) -> tensor or tuple of tensors (fp64).  Evaluates f once unperturbed (rnd = identity) and k times with every input
    multiplied by (1 + d), d uniform in [-rel, rel], and rnd(t) = t * (1 + d'), d' uniform in [-rel_mid, rel_mid] (default rel), on the
    intermediates f passes through it (and, where autograd runs through them, by (1 + d'') on their gradients).  -> (values of the unperturbed
    evaluation, element-wise max |perturbed - unperturbed| over the k runs).  The spread is the element's conditioning at the
    scale of a few fp32 roundings: an fp32 evaluation of the same formula differs from fp64 by about (spread / 16) x its rounding count."""
    g = torch.Generator().manual_seed(seed)

    rel_mid = rel if rel_mid is None else rel_mid

    def noise(t, r):
        return 1.0 + (torch.rand(t.shape, generator=g, dtype=torch.float64) * 2.0 - 1.0) * r

    as_tuple = lambda r: r if isinstance(r, tuple) else (r,)
    base = as_tuple(f(*inputs, rnd=lambda t: t))
    worst = [torch.zeros_like(b) for b in base]
    for _ in range(k):
        pin = [x * noise(x, rel) if x.is_floating_point() else x for x in inputs]
        got = as_tuple(f(*pin, rnd=lambda t: _Rounding.apply(t, noise(t, rel_mid), noise(t, rel_mid)) if t.requires_grad else t * noise(t, rel_mid)))
        worst = [torch.maximum(w, (a - b).abs()) for w, a, b in zip(worst, got, base)]
    return (base if len(base) > 1 else base[0]), (tuple(worst) if len(worst) > 1 else worst[0])
