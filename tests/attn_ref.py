"""CPU references (plain torch, fp64) for the training-mode attention core of csrc/attngrad.hip, the a-priori error bounds the GPU test holds it
to, and the nn-module reference of `train.Attention` / `train.PSABlock` -- not the product, nothing here touches the GPU.  Shared by
test_train_attn_cpu.py (which pins all of it) and test_gpu_train_attn.py.

Layout (the kernels'): qkv [B, N, nh * 128], per token [q: nh * 32 | k: nh * 32 | v: nh * 64]; out, dout, dv_add [B, N, nh * 64]; lse [B, nh, N].

  attn_fwd_ref(qkv, nh)                          -> (out, lse): S = SCALE q k^T, P = softmax_keys(S), out = P v, lse = logsumexp_keys(S)
  attn_bwd_ref(qkv, out, lse, dout, nh, dv_add)  -> dqkv: the function the kernel computes, FROM ITS OWN INPUTS: P = exp(S - lse) with the given
                                                   lse, D = sum_d dout out with the given out, dV = P^T dO (+ dv_add), dS = P o (dO V^T - D),
                                                   dQ = SCALE dS K, dK = SCALE dS^T Q.  With the exact out and lse it is autograd's gradient.
                                                   `mutate` applies one of MUTATIONS: the mistakes the bounds have to catch.
  attn_fwd_bounds / attn_bwd_bounds              per-element bounds on |device - reference|, fp64, from the rounding model below.

Rounding model of the kernels as built (u = 2^-24, u16 = 2^-8 the unit roundoff of bf16 (8 significant bits), gamma_n = n u / (1 - n u); inputs are bf16 values, so
every product of two inputs is exact in fp32):
  S        a 32-term fp32 sum in the matrix core, then one product with SCALE (the fp32 value; the reference uses the same):
             eS = SCALE gamma_32 sum |q||k| + u |S|.
  exp      e^x = v_exp_f32(fl(x * log2e_f32)): the subtraction that forms x, the constant (relative 0.93e-8 < u) and the product put 3 u |x| on the
           exponent, the instruction 1 ulp = 2 u on the result.  Results below 2^-126 may be flushed: 2^-126 absolute.
  forward  x = S - max: a common shift cancels in p / sum p.  With e = max_k (eS + 3 u |S - max|) every probability is relatively off by
             r = expm1(2 e) + 4 u (two exps) + gamma_N (the denominator's sum) + 2 u (the division, the product with it) + u16^2,
           u16^2 = 2^-16 being what the hi + lo split of P into two bf16 MFMA operands loses (P is not rounded to bf16).  The P v sum has 2 N
           terms (hi and lo): Eo = (r + gamma_2N) (P |v|), then the bf16 store: Eo += u16 (|o| + Eo).
           lse = max + log(den): E = e + gamma_N + 2 u (den) + 4 u |log den| (v_log_f32 1 ulp, ln2_f32, the product) + u |lse| (the addition).
  backward x = S - lse with the GIVEN lse: nothing cancels, the exponent error is ea = eS + 3 u |S - lse| and P is off by EP = P (expm1(ea) (1 + 2 u)
           + 2 u) + 2^-126.   dP = dO V^T: a 64-term sum (two chained MFMAs): EdP = gamma_64 sum |dO||V|.   D: 16 products added in order per
           quarter, two more additions: ED = gamma_18 sum |dO||out|.   dP - D: one subtraction: Ediff = (EdP + ED)(1 + u) + u |dP - D| -- this
           ABSOLUTE term is how the cancellation in dP - D enters every bound below; no conditioning floor is needed on top of it.
           dS = p (dP - D): EdS = (P Ediff + EP (|dP - D| + Ediff)) (1 + u) + u |dS|, then the hi + lo split: EdS += u16^2 (|dS| + EdS).
           dQ = SCALE sum_k dS K over 2 N terms (hi and lo), one product, the bf16 store:
             EdQ = SCALE (sum EdS |K| + gamma_2N sum (|dS| + EdS) |K|) (1 + u) + u |dQ|;  EdQ += u16 (|dQ| + EdQ).   dK alike over the queries.
           dV = sum_q P dO (+ dv_add): EdV = sum EP' |dO| + gamma_2N sum (P + EP') |dO| with EP' = EP + u16^2 (P + EP), + u |dV + dv_add| for the
           fp32 addition of dv_add, then the bf16 store.
No constant above is fitted: each is the count of roundings on the path it names.

The nn-module reference (fp64, NCHW, torch.autograd; blocks from dw_ref.RefBlock: Conv2d + BatchNorm2d(eps 1e-3, momentum 0.03) in .train()) is the
formula of the oracle's `_attention` / `_psa`, evaluated PLAIN (no rounding anywhere) or ROUNDED at the device's rounding points: everything
RefBlock rounds (x, weights, z, a and their gradients), the core's out, the three sums (out + pe(v), the two residuals) and the gradient sums at
the fan-outs of x, of x + attn(x) and of qkv's output (where dV meets pe's dx).  P and dS are NOT rounded (the kernels split them)."""
import torch

import dw_ref as DR
from dw_ref import _GradBf16, _q

U = 2.0 ** -24
U16 = 2.0 ** -8
TINY = 2.0 ** -126
KD, HD = 32, 64
SCALE = float(torch.tensor(KD ** -0.5, dtype=torch.float32))  # the fp32 value the kernels are handed
MUTATIONS = {"no_D": ("dq", "dk"), "scale_twice": ("dq", "dk"), "no_scale": ("dq", "dk"), "P_not_PT": ("dv",), "swap_qk": ("dq", "dk"),
             "padded_row": ("dk", "dv")}

# (N, (nh, B)) of the per-element GPU test
NS = [1, 2, 15, 16, 17, 31, 32, 33, 48, 64, 65, 169, 192]
HEADS = [(1, 1), (2, 2), (3, 1), (6, 2)]


def gamma(n):
    return n * U / (1 - n * U)


def split(t, nh, parts=(KD, KD, HD)):
    """[B, N, nh * sum(parts)] laid out [part 0 of all heads | part 1 of all heads | ...] -> tuple of [B, nh, N, part]"""
    B, N = t.shape[0], t.shape[1]
    out, o = [], 0
    for p in parts:
        out.append(t[..., o:o + nh * p].reshape(B, N, nh, p).permute(0, 2, 1, 3))
        o += nh * p
    return tuple(out)


def merge(*parts):
    """inverse of split"""
    return torch.cat([p.permute(0, 2, 1, 3).reshape(p.shape[0], p.shape[2], -1) for p in parts], dim=-1)


def core_case(N, nh, B, seed=0):
    """-> (qkv, dout, dv_add) bf16.  q, k ~ N(0, 1.5^2): S ~ N(0, 2.25^2), a peaked P that is far from one-hot"""
    g = torch.Generator().manual_seed(seed * 7919 + N * 100 + nh * 10 + B)
    qkv = torch.randn(B, N, nh * 128, generator=g)
    qkv[..., :nh * 64] *= 1.5
    dout = torch.randn(B, N, nh * 64, generator=g) * 0.5
    dv_add = torch.randn(B, N, nh * 64, generator=g) * 0.5
    return qkv.to(torch.bfloat16), dout.to(torch.bfloat16), dv_add.to(torch.bfloat16)


def attn_fwd_ref(qkv, nh):
    q, k, v = split(qkv.double(), nh)
    S = (q @ k.transpose(-2, -1)) * SCALE
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse.unsqueeze(-1))
    return merge(P @ v), lse


def attn_bwd_ref(qkv, out, lse, dout, nh, dv_add=None, mutate=None, parts=False):
    assert mutate is None or mutate in MUTATIONS
    q, k, v = split(qkv.double(), nh)
    (o,), (do,) = split(out.double(), nh, (HD,)), split(dout.double(), nh, (HD,))
    S = (q @ k.transpose(-2, -1)) * SCALE
    P = torch.exp(S - lse.double().unsqueeze(-1))
    D = (do * o).sum(-1, keepdim=True)
    dP = do @ v.transpose(-2, -1)
    qq, doo = q, do
    if mutate == "padded_row":  # a 16-row block's padded query, loaded clamped to the last row, its P row left at 1 / N instead of 0
        N = q.shape[2]
        P = torch.cat([P, torch.full_like(P[:, :, :1], 1.0 / N)], 2)
        dP, D = torch.cat([dP, dP[:, :, -1:]], 2), torch.cat([D, D[:, :, -1:]], 2)
        qq, doo = torch.cat([q, q[:, :, -1:]], 2), torch.cat([do, do[:, :, -1:]], 2)
    dS = P * (dP if mutate == "no_D" else dP - D)
    sc = {"scale_twice": SCALE * SCALE, "no_scale": 1.0}.get(mutate, SCALE)
    dq = sc * (dS @ (qq if mutate == "swap_qk" else k))
    dk = sc * (dS.transpose(-2, -1) @ (k if mutate == "swap_qk" else qq))
    dv = (P if mutate == "P_not_PT" else P.transpose(-2, -1)) @ doo
    if mutate == "padded_row":
        dq = dq[:, :, :-1]
    if dv_add is not None:
        dv = dv + split(dv_add.double(), nh, (HD,))[0]
    return (dq, dk, dv) if parts else merge(dq, dk, dv)


def _score_terms(qkv, nh):
    q, k, v = split(qkv.double(), nh)
    S = (q @ k.transpose(-2, -1)) * SCALE
    eS = SCALE * gamma(KD) * (q.abs() @ k.abs().transpose(-2, -1)) + U * S.abs()
    return q, k, v, S, eS


def attn_fwd_bounds(qkv, nh):
    """-> (E_out like out, E_lse like lse)"""
    q, k, v, S, eS = _score_terms(qkv, nh)
    N = S.shape[-1]
    mx = S.amax(-1, keepdim=True)
    e = (eS + 3 * U * (S - mx).abs()).amax(-1, keepdim=True)
    lse = torch.logsumexp(S, -1, keepdim=True)
    P = torch.exp(S - lse)
    r = torch.expm1(2 * e) + 6 * U + gamma(N) + U16 ** 2 + N * TINY
    o = P @ v
    Eo = (r + gamma(2 * N)) * (P @ v.abs())
    Eo = Eo + U16 * (o.abs() + Eo)
    El = e + gamma(N) + 2 * U + N * TINY + 4 * U * (lse - mx).abs() + U * lse.abs()
    return merge(Eo), El.squeeze(-1)


def attn_bwd_bounds(qkv, out, lse, dout, nh, dv_add=None, parts=False):
    """-> E_dqkv like dqkv (or its (dq, dk, dv) parts as [B, nh, N, .])"""
    q, k, v, S, eS = _score_terms(qkv, nh)
    (o,), (do,) = split(out.double(), nh, (HD,)), split(dout.double(), nh, (HD,))
    N = S.shape[-1]
    x = S - lse.double().unsqueeze(-1)
    P = torch.exp(x)
    ea = eS + 3 * U * x.abs()
    EP = P * (torch.expm1(ea) * (1 + 2 * U) + 2 * U) + TINY
    D = (do * o).sum(-1, keepdim=True)
    dP = do @ v.transpose(-2, -1)
    EdP = gamma(64) * (do.abs() @ v.abs().transpose(-2, -1))
    ED = gamma(18) * (do.abs() * o.abs()).sum(-1, keepdim=True)
    diff = dP - D
    Ediff = (EdP + ED) * (1 + U) + U * diff.abs()
    dS = P * diff
    EdS = (P * Ediff + EP * (diff.abs() + Ediff)) * (1 + U) + U * dS.abs()
    EdS = EdS + U16 ** 2 * (dS.abs() + EdS)
    aS = dS.abs() + EdS

    def red(E, A, M, ref):  # SCALE sum E |M| + the accumulation, the product, the store
        Eg = SCALE * (E @ M.abs() + gamma(2 * N) * (A @ M.abs())) * (1 + U) + U * ref.abs()
        return Eg + U16 * (ref.abs() + Eg)

    Edq = red(EdS, aS, k, SCALE * (dS @ k))
    Edk = red(EdS.transpose(-2, -1), aS.transpose(-2, -1), q, SCALE * (dS.transpose(-2, -1) @ q))
    EPs = EP + U16 ** 2 * (P + EP)
    dv = P.transpose(-2, -1) @ do
    Edv = EPs.transpose(-2, -1) @ do.abs() + gamma(2 * N) * ((P + EPs).transpose(-2, -1) @ do.abs())
    if dv_add is not None:
        dv = dv + split(dv_add.double(), nh, (HD,))[0]
        Edv = Edv + U * (dv.abs() + Edv)
    Edv = Edv + U16 * (dv.abs() + Edv)
    return (Edq, Edk, Edv) if parts else merge(Edq, Edk, Edv)


# ---------------------------------------------------------------------------------------------- exact cases
def sign_codes(n, g):
    """n distinct rows of 32 entries +-16, pairwise differing in at least 4 places: the first 8 places carry a row's index in binary, the other
    24 three more copies of those 8 -- two different rows differ in >= 1 of 8 places, so in d >= 4 of 32, and <q_n, k_m> = 256 (32 - 2 d) drops by
    512 d >= 2048 from the matched 8192: after SCALE the matched score leads by >= 362 > 104, and exp(-104) underflows in fp32."""
    assert n <= 256
    bits = ((torch.arange(n).unsqueeze(1) >> torch.arange(8)) & 1).double() * 2 - 1
    return (bits.repeat(1, 4) * 16.0)


def small_ints(g, *shape, hi=4):
    return torch.randint(-hi, hi + 1, shape, generator=g).double()


def onehot_case(N, nh, B):
    """-> (qkv bf16, dout bf16, pi [B, nh, N]): q_n = code n, k_m = code pi^-1(m), i.e. query n matches key pi(n); v and dout small integers."""
    g = torch.Generator().manual_seed(N * 10 + nh + B)
    codes = sign_codes(N, g)
    q = codes.expand(B, nh, N, KD)
    pi = torch.stack([torch.stack([torch.randperm(N, generator=g) for _ in range(nh)]) for _ in range(B)])
    k = torch.zeros(B, nh, N, KD, dtype=torch.float64)
    k.scatter_(2, pi.unsqueeze(-1).expand(B, nh, N, KD), q)  # k[pi(n)] = code n
    v, do = small_ints(g, B, nh, N, HD), small_ints(g, B, nh, N, HD)
    return merge(q, k, v).to(torch.bfloat16), merge(do).to(torch.bfloat16), pi


def uniform_case(N, nh, B, zero="q"):
    """q = 0 (or k = 0): S = 0, P = 1 / N; the other of q / k random, v and dout small integers."""
    g = torch.Generator().manual_seed(N + nh + B + (zero == "k"))
    r = torch.randn(B, nh, N, KD, generator=g, dtype=torch.float64)
    z = torch.zeros_like(r)
    v, do = small_ints(g, B, nh, N, HD), small_ints(g, B, nh, N, HD)
    return merge(z if zero == "q" else r, r if zero == "q" else z, v).to(torch.bfloat16), merge(do).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- the assembled reference
def qkv_perm(nh):
    """device channel i of the qkv conv is checkpoint channel perm[i] (netplan.hip's permutation, train.qkv_device_order)"""
    perm = []
    for off, n in ((0, KD), (KD, KD), (2 * KD, HD)):
        for h in range(nh):
            perm.extend(range(h * (2 * KD + HD) + off, h * (2 * KD + HD) + off + n))
    return torch.tensor(perm, dtype=torch.long)


def _core(qkv, nh, rounded):
    """oracle/yolo11_obb.py `_attention`, lines 274-277 and the v it hands to pe: qkv [B, nh * 128, H, W] in CHECKPOINT order -> (o, v) NCHW"""
    B, _, H, W = qkv.shape
    q, k, v = qkv.reshape(B, nh, 2 * KD + HD, H * W).split([KD, KD, HD], dim=2)
    attn = ((q.transpose(-2, -1) @ k) * (SCALE if rounded else KD ** -0.5)).softmax(dim=-1)
    o = (v @ attn.transpose(-2, -1)).reshape(B, nh * HD, H, W)
    return (_q(o) if rounded else o), v.reshape(B, nh * HD, H, W)


def attention_fwd(blk, x, nh, rounded):
    qkv = blk["qkv"](x, rounded)
    o, v = _core(qkv, nh, rounded)
    s = o + blk["pe"](v, rounded)
    s = _q(s) if rounded else s
    if s.requires_grad:
        s.retain_grad()
        blk["_s"] = s
    return blk["proj"](s, rounded)


def psa_fwd(blk, x, nh, rounded):
    if rounded:
        x = _GradBf16.apply(x)  # dx = bf16(d1 + d attn)
    x1 = x + attention_fwd(blk, x, nh, rounded)
    if rounded:
        x1 = _GradBf16.apply(_q(x1))  # d1 = bf16(dy + d ffn)
    y = x1 + blk["ffn1"](blk["ffn0"](x1, rounded), rounded)
    return _q(y) if rounded else y


ATTN_TAGS, PSA_TAGS = ("qkv", "proj", "pe"), ("qkv", "proj", "pe", "ffn0", "ffn1")


def block_case(kind, B, H, W, C):
    """-> (kind, nh, {tag: RefBlock}, x bf16 NHWC, dy bf16 NHWC): the seeded case of the assembled tests; kind "attn" or "psa" """
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C + (kind == "psa"))
    nh = C // 64
    blk = {"qkv": DR.RefBlock(g, C, 2 * C, 1, 1, False), "proj": DR.RefBlock(g, C, C, 1, 1, False), "pe": DR.RefBlock(g, C, C, 3, C, False)}
    if kind == "psa":
        blk.update({"ffn0": DR.RefBlock(g, C, 2 * C, 1, 1, True), "ffn1": DR.RefBlock(g, 2 * C, C, 1, 1, False)})
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    return kind, nh, blk, x, DR._grad_in(g, B, H, W, C)


def run_block(case, rounded):
    """-> {name: tensor}: out, dx (NCHW) and, per block, dW, dgamma, dbeta, rmean, rvar in checkpoint channel order; "|pe.dbeta|" is the scale
    of pe.dbeta (see block_dist)"""
    kind, nh, blk, x, dy = case
    blk.pop("_s", None)
    for b in blk.values():
        b.reset()
    xr = DR._nchw(x).clone().requires_grad_(True)
    y = (attention_fwd if kind == "attn" else psa_fwd)(blk, xr, nh, rounded)
    y.backward(DR._nchw(dy))
    out = {"out": y.detach().clone(), "dx": xr.grad.clone()}
    ds = blk.pop("_s").grad
    for t, b in blk.items():
        out.update(b.results(t + "."))
    out["|pe.dbeta|"] = ds.abs().sum((0, 2, 3)).max()
    return out


def block_dist(a, plain):
    """{name: max |a - plain| / scale}, scale = max |plain| -- the project's criterion -- for every tensor but pe.dbeta.  pe.dbeta = sum over
    the pixels of the gradient ds that proj hands back, and proj's training-mode BatchNorm makes that sum ZERO in exact arithmetic (its dz has
    zero mean per channel, and ds = W^T dz): max |plain| is rounding noise there, no scale.  Its scale is the sum it cancels from, max_c sum
    |ds| of the plain run (what test_gpu_train_dw.py's BatchNorm test divides dbeta by)."""
    scale = lambda n: float(plain["|" + n + "|"]) if "|" + n + "|" in plain else float(plain[n].double().abs().max())
    return {n: float((a[n].double().cpu() - plain[n].double()).abs().max()) / scale(n) for n in plain if not n.startswith("|")}


def fold_ref(b):
    """eval-mode BN of a RefBlock folded into its conv -> (w, bias), fp64, from its CURRENT parameters and running statistics"""
    conv, bn = b.seq[0], b.seq[1]
    f = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    return conv.weight.detach() * f.view(-1, 1, 1, 1), bn.bias.detach() - bn.running_mean * f
