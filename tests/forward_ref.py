"""fp64 reference of one *group* of the YOLO11-OBB forward and its element-wise error bound (test_forward_ref_cpu.py,
test_gpu_forward_elems.py).  Plain module, no fixtures, no GPU.

A group is the smallest piece of the graph whose inputs and outputs are all observable tensors: the uint8 tile, whatever
`ops.debug_activation` returns in the plan under test, and the head tensor.  `graph(model)` restates the topology of
oracle/yolo11_obb.py as a list of nodes over named tensors (a conv's output carries the conv's name); `Evaluator` is handed the
observable tensors and evaluates any node from the nearest observable tensors behind it, so the groups of a plan follow from what that
plan lets one observe: the GPU test lists nothing per plan.  (`hidden_in_default_plan` is a hand-kept MODEL of the 416-px default plan
for the CPU test only; nothing checks it against debug_plan and it may drift: the CPU test only needs SOME multi-layer groups.)

Reference: float64, no rounding anywhere, from the device's own input values (16-bit or fp32: exact in fp64), the weights rounded to the
storage type exactly as the engine does (`half_round`; fp32 weights for "f32") and the fp32 bias.

Bound: per element, never relative to a tensor's maximum, carried through the group as a pair (value, E) with E = 0 on observable inputs.
u = 2^-24 (fp32), u16 = 2^-11 (f16) / 2^-8 (bf16), gamma_K = K u / (1 - K u).

  conv     K = (c1/g) k^2 products plus a bias.  16-bit x 16-bit products are exact in fp32, so only the K additions and the bias addition
           round; in the fp32 path the MFMA / fmaf chain rounds once per product-and-add.  Either way (Higham, Accuracy and Stability,
           section 3.1) |z^ - z| <= gamma_{K+1} (sum |x^||w| + |b|) for any summation order, and |x^| <= |x| + E_in, so
             Ez = conv(E_in, |w|) + gamma_{K+1} (conv(|x| + E_in, |w|) + |b|).
  SiLU     silu_f(x) = x * rcp(1 + __expf(-x)), __expf(t) = v_exp_f32(t * log2(e)).  Relative errors, in units of u:
             the scaled argument -x log2(e): one rounding of the product and one of the constant: absolute 2 u |x| log2(e) on the exponent
               of two = relative 2 u |x| on the exponential;
             v_exp_f32: 1 ulp = 2 u;  both enter 1 + e weighted by e / (1 + e) < 1;
             the addition 1 + e: u;  v_rcp_f32: 1 ulp = 2 u;  the product with x: u.
           Sum: c(z) = 6 + 2 |z|.  With the propagated Ez (sup |silu'| = 1.0998 < 1.1):
             Ea = 1.1 Ez + c(z) u |silu(z)|.
           The front kernel forms x * sigmoid(x) and rounds it to 16 bit in ONE step: that drops the product's own u and is inside c(z).
           (torch's division form y / (1 + exp(-y)), which plays the device in the CPU test: exp 1 ulp, add, divide: 4 u + 2 u |z|.)
  add      residual: E = Ea + Er + u (|a + r| + Ea + Er)   (one fp32 addition).
  16 bit   wherever the device stores 16 bits (every conv / attention output except the head columns, intermediates in LDS or registers
           included: the fused kernels' headers -- bneck.hip, c3kimg.hip, dwpw.hip, front.hip, conv.hip TAIL -- all state "same rounding
           points as the separate kernels"): E += max(u16 (|a| + E), floor), floor = 2^-25 for f16 (half the subnormal spacing).
           fp32 outputs (head columns, the whole fp32 path): no such term.
  pool     MaxPool 5x5: E_out = maxpool(E) (max is 1-Lipschitz in the sup norm).
  moves    nearest upsample, concat, channel split: E moves with the values.
  input    model.0 reads half_round(fp32(v) / 255) (the kernels multiply by 1/255; the host checks that this rounds to the same 16-bit value
           for all 256 bytes -- stem_scale_is_exact) resp. fp32(v) / 255 in the fp32 path (a table of IEEE quotients): exact, E = 0.
  attn     S = scale q.k: eS = scale (gamma_kd sum |q||k| + sum (|q| Ek + Eq |k| + Eq Ek)) + 2 u |S| (scale's own rounding and the product).
           p_j = exp(S_j - max): the subtraction and the exponential's argument scaling add 3 u |S_j - max| to the exponent error; a common
           shift cancels in p_j / sum p.  With e = max_j (eS_j + 3 u |S_j - max|) every probability is relatively perturbed by at most
             r = (exp(2 e) - 1) + rho,  rho = 4 u (two exps' ulps) + gamma_N (the denominator's sum) + 2 u (1 / den, times) + u16^2
           where u16^2 is what k_attention_mfma's hi + lo split of P into two 16-bit MFMA operands leaves (nnops.hip; P is NOT rounded to 16 bit);
           for f16 the lo part may fall below the subnormal spacing: absolute 2^-24 per key on the unnormalised p (den >= 1).
             Eo = (r + gamma_N) (P |v|) + P Ev [+ 2^-24 sum_j |v_j|], then the 16-bit store.

Hidden layers.  E above is a worst case in the sup norm: conv(E_in, |w|) multiplies it by sum |w| (about 30 for a 3x3 conv of 64 channels)
per hidden layer, and behind the six hidden layers of the stride-32 C3k it reaches 1e3 .. 1e4 on values of 0.25: vacuous.  No rigorous
element-wise bound can do better (the roundings COULD all align with the signs of the weights), so groups with hidden layers also carry
a statistical bound, and the smaller of the two is used (`group_bound`).  Model (Higham & Mary, A new approach to probabilistic rounding
error analysis, SIAM J. Sci. Comput. 41, 2019): every error source p -- a layer's accumulation error, SiLU error, residual addition,
16-bit store -- is an independent mean-zero variable bounded by the same worst-case e_p as above.  The output error is, to first
order, sum_p c_p d_p with c_p the sum over paths of products of weights and SiLU slopes, and Hoeffding's inequality gives
  P(|sum c_p d_p| > LAM s) <= 2 exp(-LAM^2 / 2),  s^2 = sum c_p^2 e_p^2;  LAM = 8: 2.5e-14 per element, 1e-5 over the 4e8 elements of the suite.
s^2 is carried forward as S: S_z = conv(S_in, w^2) + e_acc^2 (which takes the paths that meet in one element as uncorrelated: exact
through 1x1 chains, an approximation where 3x3 windows overlap or a shortcut runs beside its block -- part of what LAM = 8 instead of
the 5.5 that 1e-5 over all elements needs is for), S_a = L^2 S_z + e_silu^2 with L = sup |silu'| over [z - LAM s_z, z + LAM s_z]
(the LOCAL slope), S += e^2 for the addition and the store, |x^| <= |x| + LAM s_in inside e_acc.  This is not a proof; it is the
reasoning the bound of a multi-layer group rests on, and `group_bound` asserts that the result is not vacuous.
"""
import math

import torch
import torch.nn.functional as F

import bounds
from oracle.yolo11_obb import half_round

U = 2.0 ** -24
U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f32": 0.0}
FLOOR16 = {"f16": 2.0 ** -25, "bf16": 2.0 ** -134, "f32": 0.0}


LAM = 8.0  # Hoeffding: P(|sum c_p d_p| > LAM s) <= 2 exp(-LAM^2 / 2) = 2.5e-14 per element


def gamma(k):
    return k * U / (1.0 - k * U)


def _prec(p):
    return "f32" if p in ("f32", "fp32") else p


# ---------------------------------------------------------------------------------------------- graph
def graph(m):
    """-> ordered dict name -> (op, inputs, attrs).  ops: input, conv, slice, cat, pool, up, attn."""
    G = {}
    cv = m.convs

    def conv(name, src, res=None):
        G[name] = ("conv", [src] + ([res] if res else []), {"res": res is not None})
        return name

    def sl(name, src, c0, c1):
        G[name] = ("slice", [src], {"c0": c0, "c1": c1})
        return name

    def cat(name, srcs):
        G[name] = ("cat", list(srcs), {})
        return name

    def bneck(name, src):
        return conv(name + ".cv2", conv(name + ".cv1", src), res=src)

    def c3k(name, src):
        a = conv(name + ".cv1", src)
        i = 0
        while f"{name}.m.{i}.cv1" in cv:
            a = bneck(f"{name}.m.{i}", a)
            i += 1
        b = conv(name + ".cv2", src)
        return conv(name + ".cv3", cat(name + ".cat", [a, b]))

    def c3k2(li, src):
        name = f"model.{li}"
        c = cv[name + ".cv1"].c2 // 2
        y01 = conv(name + ".cv1", src)
        ys = [sl(name + ".y0", y01, 0, c), sl(name + ".y1", y01, c, 2 * c)]
        i = 0
        while f"{name}.m.{i}.cv1" in cv:
            ys.append(c3k(f"{name}.m.{i}", ys[-1]) if f"{name}.m.{i}.cv3" in cv else bneck(f"{name}.m.{i}", ys[-1]))
            i += 1
        return conv(name + ".cv2", cat(name + ".cat", ys))

    G["x"] = ("input", ["tile"], {})
    x0 = conv("model.0", "x")
    x1 = conv("model.1", x0)
    x2 = c3k2(2, x1)
    x4 = c3k2(4, conv("model.3", x2))
    x6 = c3k2(6, conv("model.5", x4))
    x8 = c3k2(8, conv("model.7", x6))
    y = [conv("model.9.cv1", x8)]
    for i in range(3):
        G[f"model.9.pool{i}"] = ("pool", [y[-1]], {})
        y.append(f"model.9.pool{i}")
    x9 = conv("model.9.cv2", cat("model.9.cat", y))
    cp = m.psa_c
    ab = conv("model.10.cv1", x9)
    a, b = sl("model.10.a", ab, 0, cp), sl("model.10.b", ab, cp, 2 * cp)
    nh = m.psa_heads
    hd = cp // nh
    kd = hd // 2
    for i in range(m.psa_n):
        p = f"model.10.m.{i}"
        qkv = conv(p + ".attn.qkv", b)
        G[p + ".attn"] = ("attn", [qkv], {"nh": nh, "kd": kd, "hd": hd})
        G[p + ".attn.v"] = ("vslice", [qkv], {"nh": nh, "kd": kd, "hd": hd})
        pe = conv(p + ".attn.pe", p + ".attn.v", res=p + ".attn")
        b = conv(p + ".attn.proj", pe, res=b)
        b = conv(p + ".ffn.1", conv(p + ".ffn.0", b), res=b)
    x10 = conv("model.10.cv2", cat("model.10.cat", [a, b]))
    G["up13"] = ("up", [x10], {})
    x13 = c3k2(13, cat("cat13", ["up13", x6]))
    G["up16"] = ("up", [x13], {})
    x16 = c3k2(16, cat("cat16", ["up16", x4]))
    x19 = c3k2(19, cat("cat19", [conv("model.17", x16), x13]))
    x22 = c3k2(22, cat("cat22", [conv("model.20", x19), x10]))
    for i, f in enumerate((x16, x19, x22)):
        p = f"model.23.cv2.{i}"
        conv(p + ".2", conv(p + ".1", conv(p + ".0", f)))
        p = f"model.23.cv3.{i}"
        t = conv(p + ".0.1", conv(p + ".0.0", f))
        conv(p + ".2", conv(p + ".1.1", conv(p + ".1.0", t)))
        p = f"model.23.cv4.{i}"
        conv(p + ".2", conv(p + ".1", conv(p + ".0", f)))
    return G


def head_names(i):
    """the three convs whose fp32 outputs are the head columns [0:64 | 64:64+nc | 64+nc] of pyramid level i"""
    return f"model.23.cv2.{i}.2", f"model.23.cv3.{i}.2", f"model.23.cv4.{i}.2"


def is_head(name):
    return name.startswith("model.23.") and name.endswith(".2")


def qkv_device_order(nh, kd, hd):
    """device channel c of the qkv tensor holds oracle channel perm[c]: [q heads | k heads | v heads] (netplan.hip, Builder::build, C2PSA)"""
    return [h * (2 * kd + hd) + d for h in range(nh) for d in range(kd)] + [h * (2 * kd + hd) + kd + d for h in range(nh) for d in range(kd)] + \
           [h * (2 * kd + hd) + 2 * kd + d for h in range(nh) for d in range(hd)]


def silu(z):
    return z / (1.0 + torch.exp(-z))


def dsilu(z):
    sg = torch.sigmoid(z)
    return sg * (1.0 + z * (1.0 - sg))


class Evaluator:
    """obs: name -> NCHW tensor (any float dtype; "tile": uint8 NHWC).  node(name) -> (value, E, records) of that node evaluated from the
    nearest observable tensors behind it (an observable `name` itself is NOT used: it is the output under test)."""

    def __init__(self, m, precision, obs, silu_fn=silu, mutate=None, stat=False):
        self.m, self.p, self.G = m, _prec(precision), graph(m)
        self.stat = stat  # the E slot carries S = s^2 (module docstring, "hidden layers")
        self.kw = dict(silu_fn=silu_fn, mutate=mutate)
        self.obs = {k: (v if k == "tile" else v.double()) for k, v in obs.items()}
        self.memo = {}
        self.silu = silu_fn
        self.mutate = mutate or {}  # conv name -> f(w, b) -> (w, b): the emulated kernel of the CPU test
        self.u16, self.floor = U16[self.p], FLOOR16[self.p]

    def weights(self, name):
        r = self.m.convs[name]
        w = (r.w if self.p == "f32" else half_round(r.w, self.p)).double()
        b = r.b.double()
        if name in self.mutate:
            w, b = self.mutate[name](w.clone(), b.clone())
        return r, w, b

    def get(self, name):
        """(value, E, records) of `name` as an INPUT: the observed values with E = 0 where observable"""
        if name in self.obs:
            return self.obs[name], None, frozenset()
        if name not in self.memo:
            self.memo[name] = self.node(name)
        return self.memo[name]

    def twin(self):
        """the same evaluation carrying the statistical bound"""
        return Evaluator(self.m, self.p, self.obs, stat=True, **self.kw)

    def dev(self, E):
        """largest deviation an input may have: E itself, or LAM s"""
        return LAM * torch.sqrt(E) if self.stat else E

    def add(self, E, e):
        """one more independent error source bounded by e"""
        return E + e * e if self.stat else E + e

    def store16(self, a, E):
        if self.p == "f32":
            return E
        return self.add(E, torch.clamp(self.u16 * (a.abs() + self.dev(E)), min=self.floor))

    def node(self, name):
        op, ins, at = self.G[name]
        zero = lambda v, E: torch.zeros_like(v) if E is None else E
        if op == "input":
            t = torch.as_tensor(self.obs["tile"])
            if self.m.ch == 3:
                t = t.flip(-1)
            x = t.permute(0, 3, 1, 2).float() / 255.0  # IEEE fp32 quotient
            if self.p != "f32":
                x = half_round(x, self.p)
            return x.double(), None, frozenset()
        if op == "slice":
            v, E, rec = self.get(ins[0])
            return v[:, at["c0"]:at["c1"]], None if E is None else E[:, at["c0"]:at["c1"]], rec
        if op == "vslice":
            v, E, rec = self.get(ins[0])
            B, C, H, W = v.shape
            nh, kd, hd = at["nh"], at["kd"], at["hd"]
            f = lambda t: t.view(B, nh, 2 * kd + hd, H, W)[:, :, 2 * kd:].reshape(B, nh * hd, H, W)
            return f(v), None if E is None else f(E), rec
        if op == "cat":
            parts = [self.get(i) for i in ins]
            E = None if all(p[1] is None for p in parts) else torch.cat([zero(p[0], p[1]) for p in parts], 1)
            return torch.cat([p[0] for p in parts], 1), E, frozenset().union(*[p[2] for p in parts])
        if op == "pool":
            v, E, rec = self.get(ins[0])
            return F.max_pool2d(v, 5, 1, 2), None if E is None else F.max_pool2d(E, 5, 1, 2), rec | {"pool:" + name}
        if op == "up":
            v, E, rec = self.get(ins[0])
            up = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)
            return up(v), None if E is None else up(E), rec | {"up:" + name}
        if op == "attn":
            return self.attn(name, ins[0], at)
        # conv
        r, w, b = self.weights(name)
        x, Ex, rec = self.get(ins[0])
        pad = r.k // 2
        z = F.conv2d(x, w, b, stride=r.s, padding=pad, groups=r.g)
        K = (r.c1 // r.g) * r.k * r.k
        aw = w.abs()
        ax = x.abs() if Ex is None else x.abs() + self.dev(Ex)
        e_acc = gamma(K + 1) * (F.conv2d(ax, aw, None, stride=r.s, padding=pad, groups=r.g) + b.abs().view(1, -1, 1, 1))
        if Ex is None:
            Ez = e_acc * e_acc if self.stat else e_acc
        else:
            Ez = self.add(F.conv2d(Ex, w * w if self.stat else aw, None, stride=r.s, padding=pad, groups=r.g), e_acc)
        if r.act:
            a = self.silu(z)
            e_silu = (6.0 + 2.0 * z.abs()) * U * a.abs()
            if self.stat:
                rad = self.dev(Ez)
                L = torch.maximum(torch.maximum(dsilu(z - rad).abs(), dsilu(z + rad).abs()), dsilu(z).abs())
                L = torch.where((z - rad < 2.4) & (z + rad > 2.4), torch.full_like(L, 1.1), L).clamp_min(0.1)
                E = L * L * Ez + e_silu * e_silu
            else:
                E = 1.1 * Ez + e_silu
        else:
            a, E = z, Ez
        if at["res"]:
            rv, Er, rrec = self.get(ins[1])
            rec = rec | rrec
            E = E + zero(rv, Er)
            a = a + rv
            E = self.add(E, U * (a.abs() + self.dev(E)))
        if not is_head(name):
            E = self.store16(a, E)
        return a, E, rec | {name}

    def attn(self, name, src, at):
        v_, E_, rec = self.get(src)
        if self.stat:  # the analytic chain on the deviations LAM s; its result enters as ONE source bounded by Eo
            stat, self.stat = True, False
            try:
                o, Eo, rec = self.attn_worst(name, v_, None if E_ is None else LAM * torch.sqrt(E_), rec, at)
            finally:
                self.stat = stat
            return o, Eo * Eo, rec
        return self.attn_worst(name, v_, E_, rec, at)

    def attn_worst(self, name, v_, E_, rec, at):
        B, C, H, W = v_.shape
        N = H * W
        nh, kd, hd = at["nh"], at["kd"], at["hd"]
        sp = lambda t: t.reshape(B, nh, 2 * kd + hd, N).split([kd, kd, hd], dim=2)
        q, k, v = sp(v_)
        scale = float(torch.tensor(kd ** -0.5, dtype=torch.float32))  # the fp32 value the kernel is handed
        qt = q.transpose(-2, -1)
        S = (qt @ k) * scale  # [B, nh, query, key]
        eS = scale * gamma(kd) * (qt.abs() @ k.abs()) + 2 * U * S.abs()
        if E_ is not None:
            Eq, Ek, Ev = sp(E_)
            eS = eS + scale * (qt.abs() @ Ek + Eq.transpose(-2, -1) @ (k.abs() + Ek))
        mx = S.amax(-1, keepdim=True)
        e = (eS + 3 * U * (S - mx).abs()).amax(-1, keepdim=True)
        P = torch.softmax(S, -1)
        r = torch.expm1(2 * e) + 6 * U + gamma(N) + self.u16 ** 2
        av = v.abs().transpose(-2, -1)  # [B, nh, key, hd]
        o = P @ v.transpose(-2, -1)
        Eo = (r + gamma(N)) * (P @ av)
        if E_ is not None:
            Eo = Eo + P @ Ev.transpose(-2, -1)
        if self.p == "f16":
            Eo = Eo + 2.0 ** -24 * av.sum(-2, keepdim=True)
        o = o.transpose(-2, -1).reshape(B, nh * hd, H, W)
        Eo = Eo.transpose(-2, -1).reshape(B, nh * hd, H, W)
        return o, self.store16(o, Eo), rec | {"attn:" + name}


def check_group(what, got, ref, bound):
    """bounds._check (|got - ref| <= bound for EVERY element, printing the worst |err| / bound: the measured margin) -> that worst ratio"""
    got = got.double().cpu().reshape(ref.shape)
    d = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    worst = float(torch.where(d == 0, torch.zeros_like(d), d / bound).max()) if d.numel() else 0.0
    bounds._check(what, got, ref, bound)
    return worst


def vacuous_above(n, u16):
    """largest median bound, relative to the median |ref|, a group may have and still count as a check: 1/2 -- beyond that an all-zero
    output would pass for most elements.  (What the bounds actually are, in units of one 16-bit rounding, is printed per group.)"""
    return 0.5


def group_bound(ev, name, tw=None):
    """(fp64 reference, bound, records) of the group that ends at `name`: the worst-case E; for a group with hidden layers the smaller of
    E and LAM s, asserted NOT to be vacuous (a bound that says nothing cannot count as coverage): see vacuous_above"""
    ref, E, rec = ev.node(name)
    assert E is not None, name
    n = sum(r in ev.m.convs for r in rec)
    if n > 1:
        _, S, _ = (tw or ev.twin()).node(name)
        E = torch.minimum(E, LAM * torch.sqrt(S))
        rel = float(E.median()) / float(ref.abs().median())
        print(f"  {name}: {n} convs, median bound = {rel:.2e} x median |ref|" + (f" = {rel / ev.u16:.0f} u16" if ev.u16 else ""))
        assert rel <= vacuous_above(n, ev.u16), f"{name}: vacuous bound: median {float(E.median()):.3e} on values of median {float(ref.abs().median()):.3e} ({n} convs)"
    return ref, E, rec


def check_all(ev, outputs, label="", got=None):
    """every tensor of `outputs` (names observable in ev.obs) against its group -> ({name: worst ratio}, set of records inside checked groups)"""
    ratios, covered = {}, set()
    tw = ev.twin()
    for name in outputs:
        ref, E, rec = group_bound(ev, name, tw)
        g = ev.obs[name] if got is None else got[name]
        members = sorted(rec)
        what = f"{label}{name} <- [{len(members)}] {'+'.join(n.replace('model.', '') for n in members if n != name)}"
        ratios[name] = check_group(what, g, ref, E)
        covered |= rec
    return ratios, covered


def hidden_in_default_plan(m):
    """the intermediates the default plan of a 416-px tile never writes or overwrites in place (the CPU test forms its multi-layer groups
    by hiding them): front, Bottleneck + closing 1x1, stride-2 conv + cv1, the per-image C3k, DW -> 1x1 (-> head 1x1), the fused head
    tails, the merged C3k member and the PSA block's in-place updates."""
    h = {"model.0", "model.1", "model.3", "model.10.cv1", "model.10.b", "model.6.m.0.cv1"}
    for li in (2, 4, 16):
        h |= {f"model.{li}.m.0.cv1", f"model.{li}.m.0.cv2"}
    for li in (8, 22):
        if m.convs[f"model.{li}.m.0.cv1"].c1 != 128:  # c3kimg_supported: the n widths only (128 -> 64 -> 128); other scales keep the block's layers observable
            continue
        h |= {n for n in m.convs if n.startswith(f"model.{li}.m.0.") and not n.endswith(".cv3")}
    for i in range(m.psa_n):
        h.add(f"model.10.m.{i}.attn.proj")
    for i in range(3):
        h |= {f"model.23.cv2.{i}.1", f"model.23.cv4.{i}.1", f"model.23.cv3.{i}.0.0", f"model.23.cv3.{i}.1.0", f"model.23.cv3.{i}.1.1"}
    return h
