"""fp64 references and per-element error bounds for the trainer-update kernels (csrc/trainupd.hip: gradient norm, clip coefficient, the clipped
multi-group optimiser step, gradient accumulation, EMA) and for train.Schedule / ModelEMA / TrainerUpdate.  Used by test_gpu_train_update.py
(against the device) and test_train_update_cpu.py (host side).  The optimiser references are train_loss_ref.sgd_ref / adamw_ref.  u = 2^-24.

Every bound is derived, none is measured:
  * total_norm: the device squares and sums in double and rounds ONCE to fp32, so |total_norm - ref| <= u ref from that rounding; the double sum of
    n squares carries at most n 2^-53 in relative terms (1e5 elements: 1e-11), far inside the second u.  Bound: 2 u ref.
  * coef = min(1, max_norm / (total + 1e-6)): again one fp32 rounding of a double value: u coef (the rounding error is at most u 2^e for a
    value in [2^e, 2^(e+1)), so the double arithmetic's own few 2^-53 fit inside u coef everywhere but at a power of two).
  * EMA e' = fl(fl(e d') + fl(o' s)) with d' = fl32(d), o' = fl32(1 - d): the two constants and the three operations round by u each; every
    term of the result carries at most three of them: (1 + u)^3 - 1 < 4 u on d |e| + (1 - d) |s|.
  * accumulate: one fp32 add: exact against torch's fp32 add."""
import math

import numpy as np
import torch

from bounds import U

LENGTHS = (0, 1, 3, 4, 5, 4095, 4096, 4097, 100003)
# every length above, an empty segment in each position, a lone 1-element segment, more than one slab and a slab with a scalar tail
TRIPLES = [(1, 0, 4097), (3, 4, 5), (4095, 4096, 100003), (0, 100003, 1), (0, 1, 0)]
assert {n for t in TRIPLES for n in t} == set(LENGTHS)
MAX_NORMS = (10.0, 1e-3, 1e30)


def triple_id(t):
    return "-".join(str(n) for n in t)


def grads_of(sizes, seed, scale=1.0):
    """fp32 gradient segments: normal values times `scale`, a few exact zeros"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        v = torch.randn(n, generator=g) * scale
        v[3::11] = 0.0
        out.append(v)
    return out


def norm_ref(grads):
    """-> (total = sqrt(sum g^2) in fp64, its bound 2 u total)"""
    total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    return total, 2 * U * total


def coef_ref(total, max_norm):
    """-> (coef in fp64, bound); NaN total: NaN; infinite total: 0"""
    c = max_norm / (total + 1e-6)
    c = c if math.isnan(c) else min(1.0, c)
    return c, U * abs(c)


def ema_ref(e, s, d):
    """-> (e d + (1 - d) s in fp64 with the double d, bound 4 u (d |e| + (1 - d) |s|))"""
    e, s = e.double(), s.double()
    return e * d + (1.0 - d) * s, 4 * U * (d * e.abs() + (1.0 - d) * s.abs()) + 1e-45


def ema_shortcut_f32(e, s, d):
    """the update with 1.0f - (float)d in place of (float)(1 - d), in fp32 on the CPU: what the bound must catch at d = 0.9999"""
    df = np.float32(d)
    omd = np.float32(1.0) - df
    return (e.numpy() * df + omd * s.numpy()).astype(np.float32)


def ema_torch_f32(e, s, d):
    """torch's own sequence in fp32 (ultralytics ModelEMA.update: v *= d; v += (1 - d) * s): the calibration"""
    v = e.clone()
    v.mul_(d)
    v.add_((1.0 - d) * s)
    return v


def ema_decay(updates, decay=0.9999, tau=2000.0):
    return decay * (1.0 - math.exp(-updates / tau))
