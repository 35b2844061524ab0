"""CPU checks of the training-mode attention slice (csrc/attngrad.hip, `train.Attention` / `train.PSABlock`): the fp64 references of
tests/attn_ref.py against torch.autograd and against the oracle's `_psa`, the boundary (header, ctypes signatures, ops wrappers, train classes),
the proof that the a-priori bounds catch the mistakes they are there for, the exactness of the exact cases, and the rounded-against-plain
measurement that sets the tolerances of the assembled GPU tests.  No GPU."""
import os
import re

import pytest
import torch

import attn_ref as AR
import dw_ref as DR
from conftest import ROOT

SHAPES = [(2, 1, 1), (3, 2, 1), (16, 1, 2), (17, 3, 1), (33, 2, 2), (169, 2, 1)]  # (N, nh, B)
NEW = ["obb_attn_fwd_bf16", "obb_attn_bwd_bf16", "obb_add_bf16"]


@pytest.mark.parametrize("N,nh,B", [(1, 1, 1)] + SHAPES)
def test_reference_backward_equals_autograd(N, nh, B):
    """attn_bwd_ref, fed the exact out and lse, is autograd's gradient of the plain three-step formula (matmul, softmax, matmul) to 1e-12."""
    qkv, dout, dv_add = AR.core_case(N, nh, B)
    x = qkv.double().requires_grad_(True)
    q, k, v = AR.split(x, nh)
    o = AR.merge(torch.softmax((q @ k.transpose(-2, -1)) * AR.SCALE, -1) @ v)
    o.backward(dout.double())
    out, lse = AR.attn_fwd_ref(qkv, nh)
    assert float((out - o.detach()).abs().max()) <= 1e-12 * float(o.detach().abs().max())
    got = AR.attn_bwd_ref(qkv, out, lse, dout, nh)
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    extra = AR.attn_bwd_ref(qkv, out, lse, dout, nh, dv_add=dv_add) - got
    want = torch.zeros_like(extra)
    want[..., nh * 64:] = dv_add.double()
    assert float((extra - want).abs().max()) <= 1e-12


def _eval_blocks(blk):
    for b in blk.values():
        b.seq.eval()


def test_module_reference_in_eval_equals_the_oracle_psa():
    """The nn-module restatement in .eval(), against oracle/yolo11_obb.py `_psa` fed the same blocks with their BN folded -- and the qkv block
    taken through the device permutation and back, as train.Attention holds and folds it."""
    from oracle.yolo11_obb import Yolo11OBB
    case = AR.block_case("psa", 2, 5, 4, 128)
    _, nh, blk, x, _ = case
    _eval_blocks(blk)
    try:
        with torch.no_grad():
            want = AR.psa_fwd(blk, DR._nchw(x), nh, False)
        net = Yolo11OBB("n", nc=12, ch=3, seed=0)
        assert net.psa_heads == nh and net.psa_c == 128
        net.mode, net.bf16, net.taps, net.calib = "fp64", False, None, False
        perm = AR.qkv_perm(nh)
        inv = torch.argsort(perm)
        assert sorted(perm.tolist()) == list(range(nh * 128)) and perm.tolist() != list(range(nh * 128))
        for tag, name in (("qkv", "attn.qkv"), ("proj", "attn.proj"), ("pe", "attn.pe"), ("ffn0", "ffn.0"), ("ffn1", "ffn.1")):
            w, b = AR.fold_ref(blk[tag])
            if tag == "qkv":
                w, b = w[perm][inv], b[perm][inv]
            r = net.convs["model.10.m.0." + name]
            assert tuple(r.w.shape) == tuple(w.shape) and r.act == blk[tag].act
            r.w, r.b = w, b
        got = net._psa("model.10.m.0", DR._nchw(x))
    finally:
        for b in blk.values():
            b.seq.train()
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_qkv_permutation_is_the_engines():
    """attn_ref.qkv_perm / train.qkv_device_order restate the loop of csrc/netplan.hip: [q_h0.. | k_h0.. | v_h0..] <- per-head [q | k | v]."""
    import oriented_object_detection_amd  # noqa: F401
    import oriented_object_detection_amd.train as TR
    for nh in (1, 2, 3, 6):
        kd, hd = 32, 64
        perm = [0] * (nh * 128)
        for hh in range(nh):
            src0 = hh * (2 * kd + hd)
            for d in range(kd):
                perm[hh * kd + d] = src0 + d
                perm[nh * kd + hh * kd + d] = src0 + kd + d
            for d in range(hd):
                perm[2 * nh * kd + hh * hd + d] = src0 + 2 * kd + d
        assert AR.qkv_perm(nh).tolist() == perm and TR.qkv_device_order(nh).tolist() == perm


@pytest.mark.parametrize("N,nh,B", SHAPES)
@pytest.mark.parametrize("mutation", sorted(AR.MUTATIONS))
def test_bounds_catch_mutations(mutation, N, nh, B):
    """Each mistake, made in the fp64 reference itself, leaves the bound at some element of each output it is named for; the unmutated
    reference with out and lse rounded as the device hands them over (bf16, fp32) stays inside, so the bound is not beaten by its own inputs."""
    qkv, dout, dv_add = AR.core_case(N, nh, B)
    out, lse = AR.attn_fwd_ref(qkv, nh)
    out, lse = out.to(torch.bfloat16), lse.float()
    ref = dict(zip(("dq", "dk", "dv"), AR.attn_bwd_ref(qkv, out, lse, dout, nh, dv_add, parts=True)))
    bad = dict(zip(("dq", "dk", "dv"), AR.attn_bwd_ref(qkv, out, lse, dout, nh, dv_add, mutate=mutation, parts=True)))
    E = dict(zip(("dq", "dk", "dv"), AR.attn_bwd_bounds(qkv, out, lse, dout, nh, dv_add, parts=True)))
    for name in AR.MUTATIONS[mutation]:
        worst = float(((bad[name] - ref[name]).abs() / E[name]).max())
        print(f"{mutation} N = {N}: {name} leaves the bound by {worst:.1f} x")
        assert worst > 1, (mutation, name, worst)
    for name in ("dq", "dk", "dv"):  # the bound is a few bf16 roundings of the result wide, not orders of magnitude
        rel = float((E[name] / (ref[name].abs() + E[name].mean())).median())
        assert rel < 0.02, (name, rel)


@pytest.mark.parametrize("N", [16, 17, 169])
def test_exact_cases_are_exact_in_fp32(N):
    """The exact-case inputs evaluated in fp32 on the CPU: P bit-equal to one-hot (sign codes) resp. to 1 / N (q = 0, N = 16)."""
    nh, B = 2, 1
    qkv, _, pi = AR.onehot_case(N, nh, B)
    q, k, _ = AR.split(qkv.float(), nh)
    S = (q @ k.transpose(-2, -1)) * torch.tensor(AR.SCALE, dtype=torch.float32)
    assert S.dtype == torch.float32
    top2 = S.topk(min(2, N), -1).values
    assert N == 1 or float((top2[..., 0] - top2[..., 1]).min()) > 104
    lse = torch.logsumexp(S, -1, keepdim=True)
    P = torch.exp(S - lse)
    hot = torch.zeros_like(P).scatter_(-1, pi.unsqueeze(-1), 1.0)
    assert torch.equal(P, hot)
    assert torch.equal(lse.squeeze(-1), S.amax(-1))
    if N == 16:
        qkv, _ = AR.uniform_case(16, nh, B, "q")
        q, k, _ = AR.split(qkv.float(), nh)
        S = (q @ k.transpose(-2, -1)) * torch.tensor(AR.SCALE, dtype=torch.float32)
        assert bool((S == 0).all())
        lse = torch.log(torch.exp(S).sum(-1, keepdim=True))
        # the kernels' own path: exp2(x * log2e), log2(x) * ln2 with fp32 constants
        l2e, ln2 = torch.tensor(1.4426950408889634, dtype=torch.float32), torch.tensor(0.6931471805599453, dtype=torch.float32)
        lse_k = torch.log2(torch.exp2(S * l2e).sum(-1, keepdim=True)) * ln2
        for l in (lse, lse_k):
            assert torch.equal(torch.exp(S - l), torch.full_like(S, 1.0 / 16))
            assert torch.equal(torch.exp2((S - l) * l2e), torch.full_like(S, 1.0 / 16))


def test_attn_boundary_is_declared_bound_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "obbhip.h")).read()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    import oriented_object_detection_amd.train as TR
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/obbhip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(",")), name
    for op in ("attn_fwd", "attn_bwd", "add_bf16"):
        assert hasattr(torch.ops.obbhip, op), f"torch.ops.obbhip.{op} is not registered"
    assert all(callable(getattr(TR, n, None)) for n in ("Attention", "PSABlock", "qkv_device_order"))
    q = torch.zeros(1, 16, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="no CPU path"):  # no quiet fall-back
        ops.attn_fwd_bf16(q, 1)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.attn_bwd_bf16(q, q[..., :64].contiguous(), torch.zeros(1, 1, 16), q[..., :64].contiguous(), 1)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.add_bf16(q, q)
    with pytest.raises(ValueError, match="nh = 2 heads"):
        TR.Attention(TR.ParamGroups(), (torch.zeros(128, 64, 1, 1),), (torch.zeros(64, 64, 1, 1),), (torch.zeros(64, 1, 3, 3),), 2)
    g = TR.ParamGroups()
    blk = TR.ConvBN(g, torch.zeros(8, 8, 1, 1), act=False)
    assert blk.act is False and TR.ConvBN(g, torch.zeros(8, 8, 1, 1)).act is True


# The tolerances of the assembled GPU tests: e = max |rounded - plain| / max |plain| per tensor (test_train_dw_cpu.py explains the criterion),
# measured here at the bf16 rounding points of the device; the GPU test recomputes e from the same functions and requires the device within 2 e
# of plain.  E_F32 is the same measurement with every rounding point at float32 instead: the floor that the fp64 restatement itself
# leaves, five orders below -- what the device is measured against is its bf16 storage, not the reference.
E_BLOCKS = {
    ("attn", 2, 13, 13, 128): {"out": 5.30e-3, "dx": 5.57e-3, "qkv.dW": 4.32e-3, "qkv.dgamma": 1.94e-2, "qkv.dbeta": 8.36e-3, "qkv.rmean": 4.44e-5,
                               "qkv.rvar": 7.82e-5, "proj.dW": 5.02e-3, "proj.dgamma": 4.90e-3, "proj.dbeta": 0.0, "proj.rmean": 2.21e-4,
                               "proj.rvar": 1.80e-4, "pe.dW": 4.07e-3, "pe.dgamma": 3.05e-3, "pe.dbeta": 5.53e-4, "pe.rmean": 2.24e-4, "pe.rvar": 3.11e-4},
    ("attn", 2, 4, 4, 192): {"out": 6.92e-3, "dx": 8.77e-3, "qkv.dW": 6.17e-3, "qkv.dgamma": 1.04e-2, "qkv.dbeta": 5.76e-3, "qkv.rmean": 2.48e-4,
                             "qkv.rvar": 1.71e-4, "proj.dW": 8.01e-3, "proj.dgamma": 5.19e-3, "proj.dbeta": 0.0, "proj.rmean": 3.44e-4,
                             "proj.rvar": 4.72e-4, "pe.dW": 4.56e-3, "pe.dgamma": 5.45e-3, "pe.dbeta": 1.05e-3, "pe.rmean": 3.18e-4, "pe.rvar": 7.81e-4},
    # (proj.dbeta / ffn1.dbeta of the block that ends the stack are plain sums of the incoming gradient, which no rounding point touches: e = 0)
    ("psa", 2, 13, 13, 128): {"out": 6.72e-3, "dx": 5.54e-3, "qkv.dW": 6.72e-3, "qkv.dgamma": 2.04e-2, "qkv.dbeta": 1.42e-2, "qkv.rmean": 7.45e-5,
                              "qkv.rvar": 6.62e-5, "proj.dW": 4.89e-3, "proj.dgamma": 6.87e-3, "proj.dbeta": 2.62e-3, "proj.rmean": 2.60e-4,
                              "proj.rvar": 1.40e-4, "pe.dW": 6.50e-3, "pe.dgamma": 6.62e-3, "pe.dbeta": 3.50e-4, "pe.rmean": 2.32e-4, "pe.rvar": 6.11e-4,
                              "ffn0.dW": 6.99e-3, "ffn0.dgamma": 9.42e-3, "ffn0.dbeta": 1.03e-2, "ffn0.rmean": 1.74e-4, "ffn0.rvar": 2.93e-4,
                              "ffn1.dW": 6.04e-3, "ffn1.dgamma": 6.45e-3, "ffn1.dbeta": 0.0, "ffn1.rmean": 1.64e-4, "ffn1.rvar": 4.35e-5},
}


def _e(case):
    plain, rounded = AR.run_block(case, False), AR.run_block(case, True)
    return AR.block_dist(rounded, plain)


@pytest.mark.parametrize("kind,B,H,W,C", list(E_BLOCKS))
def test_rounded_against_plain_blocks(kind, B, H, W, C, monkeypatch):
    case = AR.block_case(kind, B, H, W, C)
    e = _e(case)
    print(f"{kind} {B}x{H}x{W}x{C} bf16: " + ", ".join(f"{n} {v:.2e}" for n, v in e.items()))
    monkeypatch.setattr(DR, "bf16", lambda t: t.float().to(t.dtype))
    e32 = _e(case)
    print(f"{kind} {B}x{H}x{W}x{C} float32: " + ", ".join(f"{n} {v:.2e}" for n, v in e32.items()))
    tags = AR.ATTN_TAGS if kind == "attn" else AR.PSA_TAGS
    assert set(e) == {"out", "dx"} | {f"{t}.{s}" for t in tags for s in ("dW", "dgamma", "dbeta", "rmean", "rvar")}
    for n in e:
        assert e32[n] <= 1e-5, (n, e32[n])
        assert e[n] <= 0.05, (n, e[n])
        assert e[n] == 0 or e[n] >= 100 * e32[n], (n, e[n], e32[n])
    measured = E_BLOCKS[(kind, B, H, W, C)]
    if measured is not None:
        for n, v in e.items():
            assert measured[n] / 1.5 <= v <= measured[n] * 1.5 or (measured[n] == 0 and v == 0), (n, v, measured[n])
