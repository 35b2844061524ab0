"""CPU references for the channel-window kernel of csrc/routegrad.hip (obb_chanwin_bf16) and for the composite training blocks built on it
(`train.Bottleneck` / `C3k` / `C3k2` / `C2PSA`) -- not the product, nothing here touches the GPU.  Shared by test_train_blocks_cpu.py (which pins
the restatements against plain nn.Modules and shows that the bound separates a correct stand-in from planted mistakes) and test_gpu_train_blocks.py.

  chanwin_ref(src, s0, n, dst, d0, add, a0)   torch slicing; with add (s.float() + a.float()).to(bfloat16): the exact answer, not an approximation

The blocks are restated over `route_ref.RefConvBN` leaves (fp32 parameters; C2PSA's PSABlocks are attn_ref's dicts of dw_ref.RefBlock under
attn_ref.psa_fwd) and evaluated by `run(case, plain)` under torch.autograd, NCHW:

  plain = False   fp32 at the device's rounding points: RefConvBN(x, grad_bf16=True) (weights, z, a; dz and the conv's dx on the way back), the
                  residual sums and their gradient sums (Bottleneck), the sum of C3k's two dx, the gradient sum at every C3k2 concat member that
                  feeds a further member, the PSA reference ROUNDED (fp64 arithmetic on bf16 values)
  plain = True    the same graph in fp64 with no rounding point at all, from the same parameters and running statistics

A `spec` is a dict {"kind", leaves..., "m": [member specs]}; `leaves(spec)` lists (checkpoint-relative name, leaf) in train.py's registration order;
`module_args` / `build_module` hand the leaves' tensors to the constructors of train.py (or of a stand-in namespace with the same signatures).

The bound of the block tests: figure = max |got - ref| / max |ref| per quantity against run(case, False); bound = max(route_ref.FLOOR[kind],
4 x grain), grain = the same figure of run(case, False) against run(case, True).  Why 4: the device's bf16 roundings land independently of the
reference's, so two such evaluations can differ by twice the grain, and a further factor 2 covers the matrix cores' summation order against
torch's.  Nothing in the bound comes from the device.  Three quantities have a vacuous bound: the dbeta of a PSABlock's proj, pe and ffn.1 are sums that
cancel to zero in exact arithmetic (the next BatchNorm's dz has zero mean per channel; attn_ref.block_dist), so their fp64 values are noise and
their grain enormous; the tolerance-free composition test and test_gpu_train_attn.py cover them."""
import torch
import torch.nn.functional as F

import attn_ref as AR
import dw_ref as DR
import route_ref as RR
from route_ref import RefConvBN, _GradBf16, q

EPS, MOM = RR.EPS, RR.MOM
PSA_NAMES = {"qkv": "attn.qkv", "proj": "attn.proj", "pe": "attn.pe", "ffn0": "ffn.0", "ffn1": "ffn.1"}


def chanwin_ref(src, s0, n, dst=None, d0=0, add=None, a0=0):
    """-> the whole of dst after the call (a dense [..., n] tensor when dst is None); dst itself is not modified"""
    w = src[..., s0:s0 + n]
    if add is not None:
        w = (w.float() + add[..., a0:a0 + n].float()).to(torch.bfloat16)
    if dst is None:
        return w.clone().contiguous()
    out = dst.clone()
    out[..., d0:d0 + n] = w
    return out


# ---------------------------------------------------------------------------------------------- specs
def make_bottleneck(g, c, c_):
    return {"kind": "bottleneck", "cv1": RefConvBN(g, c, c_, 3), "cv2": RefConvBN(g, c_, c, 3)}


def make_c3k(g, c1, c2, n=2):
    c_ = c2 // 2
    return {"kind": "c3k", "cv1": RefConvBN(g, c1, c_), "cv2": RefConvBN(g, c1, c_), "cv3": RefConvBN(g, 2 * c_, c2),
            "m": [make_bottleneck(g, c_, c_) for _ in range(n)]}


def make_c3k2(g, c1, c2, n, c3k, e):
    c = int(c2 * e)
    return {"kind": "c3k2", "c3k": c3k, "cv1": RefConvBN(g, c1, 2 * c), "cv2": RefConvBN(g, (2 + n) * c, c2),
            "m": [make_c3k(g, c, c, 2) if c3k else make_bottleneck(g, c, c // 2) for _ in range(n)]}


def make_c2psa(g, c1, n=1):
    c = c1 // 2
    psa = lambda: {"qkv": DR.RefBlock(g, c, 2 * c, 1, 1, False), "proj": DR.RefBlock(g, c, c, 1, 1, False), "pe": DR.RefBlock(g, c, c, 3, c, False),
                   "ffn0": DR.RefBlock(g, c, 2 * c, 1, 1, True), "ffn1": DR.RefBlock(g, 2 * c, c, 1, 1, False)}
    return {"kind": "c2psa", "nh": c // 64, "cv1": RefConvBN(g, c1, 2 * c), "cv2": RefConvBN(g, 2 * c, c1), "m": [psa() for _ in range(n)]}


def leaves(spec, prefix=""):
    """[(name, RefConvBN or dw_ref.RefBlock)] in train.py's registration order"""
    kind = spec.get("kind", "psa")
    if kind == "psa":
        return [(prefix + PSA_NAMES[t], spec[t]) for t in AR.PSA_TAGS]
    own = [(prefix + n, spec[n]) for n in ("cv1", "cv2", "cv3") if n in spec]
    for i, m in enumerate(spec.get("m", [])):
        own += leaves(m, f"{prefix}m.{i}.")
    return own


def leaf_args(leaf, dev=lambda t: t):
    """(w, gamma, beta, running_mean, running_var) of a leaf as it stands, through dev"""
    if isinstance(leaf, RefConvBN):
        src = (leaf.w, leaf.bn.weight, leaf.bn.bias, leaf.bn.running_mean, leaf.bn.running_var)
    else:
        src = leaf.init
    return tuple(dev(t.detach().clone().float()) for t in src)


def module_args(spec, dev=lambda t: t):
    """the positional arguments of the block's constructor in train.py after `groups`"""
    A = lambda n: leaf_args(spec[n], dev)
    kind = spec["kind"]
    if kind == "bottleneck":
        return (A("cv1"), A("cv2"))
    if kind == "c3k":
        return (A("cv1"), A("cv2"), A("cv3"), [module_args(m, dev) for m in spec["m"]])
    if kind == "c3k2":
        return (A("cv1"), A("cv2"), [module_args(m, dev) for m in spec["m"]], spec["c3k"])
    return (A("cv1"), A("cv2"), [tuple(leaf_args(m[t], dev) for t in AR.PSA_TAGS) for m in spec["m"]], spec["nh"])


def build_module(TR, groups, spec, dev=lambda t: t):
    cls = {"bottleneck": "Bottleneck", "c3k": "C3k", "c3k2": "C3k2", "c2psa": "C2PSA"}[spec["kind"]]
    return getattr(TR, cls)(groups, *module_args(spec, dev), EPS, MOM)


# ---------------------------------------------------------------------------------------------- evaluation
class _Run:
    """One evaluation: the leaves it went through with what their results are read from."""

    def __init__(self, plain):
        self.plain, self.used = plain, []

    def conv(self, R, x):
        if not self.plain:
            for p in R.params():
                p.grad = None
            self.used.append((R, None))
            return R(x, grad_bf16=True)
        w, gm, bt = (t.detach().double().clone().requires_grad_(True) for t in R.params())
        rm, rv = R.bn.running_mean.double().clone(), R.bn.running_var.double().clone()
        self.used.append((R, (w, gm, bt, rm, rv)))
        return F.silu(F.batch_norm(F.conv2d(x, w, stride=R.s, padding=R.k // 2), rm, rv, gm, bt, True, MOM, EPS))

    def G(self, t):
        return t if self.plain else _GradBf16.apply(t)

    def Q(self, t):
        return t if self.plain else q(t)

    def bottleneck(self, sp, x):
        x = self.G(x)  # dx = bf16(dy + cv1's dx)
        return self.Q(x + self.conv(sp["cv2"], self.conv(sp["cv1"], x)))

    def c3k(self, sp, x):
        x = self.G(x)  # dx = bf16(cv1's dx + cv2's dx)
        a = self.conv(sp["cv1"], x)
        for m in sp["m"]:
            a = self.bottleneck(m, a)
        return self.conv(sp["cv3"], torch.cat([a, self.conv(sp["cv2"], x)], 1))

    def c3k2(self, sp, x):
        y0, cur = self.conv(sp["cv1"], x).chunk(2, 1)
        ys = [y0]
        for m in sp["m"]:
            cur = self.G(cur)  # the gradient of a member's input: bf16(dcat's window + the member's dx)
            ys.append(cur)
            cur = (self.c3k if sp["c3k"] else self.bottleneck)(m, cur)
        return self.conv(sp["cv2"], torch.cat(ys + [cur], 1))

    def c2psa(self, sp, x):
        c = sp["nh"] * 64
        a, b = self.conv(sp["cv1"], x).split((c, c), 1)
        b = b.double()
        for m in sp["m"]:
            b = AR.psa_fwd(m, b, sp["nh"], not self.plain)
        return self.conv(sp["cv2"], torch.cat([a, b.to(a.dtype)], 1))


def run(case, plain):
    """case = (spec, x bf16 NHWC, dy bf16 NHWC) -> {name: tensor}: out, dx (NCHW) and per leaf <name>.dW / dgamma / dbeta / rmean / rvar.  The
    rounded evaluation updates the RefConvBN leaves' running statistics in place (their live tensors are their state); the plain one changes
    nothing, so run(case, True) comes first.  RefBlock leaves start from their `init` in both."""
    spec, x, dy = case
    dt = torch.float64 if plain else torch.float32
    r = _Run(plain)
    psa = [m for m in spec.get("m", []) if "kind" not in m]
    for m in psa:
        m.pop("_s", None)
        for b in m.values():
            b.reset()
    xr = x.to(dt).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = getattr(r, spec["kind"])(spec, xr)
    y.backward(dy.to(dt).permute(0, 3, 1, 2))
    for m in psa:
        m.pop("_s", None)
    out = {"out": y.detach().clone(), "dx": xr.grad.clone()}
    twins = {id(R): t for R, t in r.used}
    assert len(twins) == len(r.used)
    for name, leaf in leaves(spec):
        if not isinstance(leaf, RefConvBN):
            out.update(leaf.results(name + "."))
            continue
        t = twins[id(leaf)]
        vals = (leaf.w.grad, leaf.bn.weight.grad, leaf.bn.bias.grad, leaf.bn.running_mean, leaf.bn.running_var) if t is None else \
            (t[0].grad, t[1].grad, t[2].grad, t[3], t[4])
        out.update({f"{name}.{k}": v.detach().clone() for k, v in zip(("dW", "dgamma", "dbeta", "rmean", "rvar"), vals)})
    return out


def collect(mod, out, dx, invs=None):
    """A block of train.py (or a stand-in with the same `named_blocks`) after forward + backward -> {name: tensor} under run()'s names.  invs:
    {leaf name: device channel order -> checkpoint order} (the qkv blocks of C2PSA)."""
    nchw = lambda t: t.double().cpu().permute(0, 3, 1, 2)
    got = {"out": nchw(out), "dx": nchw(dx)}
    for name, d in mod.named_blocks():
        inv = (invs or {}).get(name)
        r = {"dW": d.dw, "dgamma": d.dgamma, "dbeta": d.dbeta, "rmean": d.running_mean, "rvar": d.running_var}
        got.update({f"{name}.{k}": (t if inv is None else t[inv.to(t.device)]).detach().clone() for k, t in r.items()})
    return got


def figures(a, ref):
    """{name: max |a - ref| / max |ref|}"""
    assert set(a) == set(ref), set(a) ^ set(ref)
    return {n: DR.rel_dist(a[n].cpu().reshape(ref[n].shape), ref[n]) for n in ref}


def bounds(rounded, plain):
    """{name: max(FLOOR[kind], 4 x grain)} from the two references alone"""
    return {n: max(RR.FLOOR[n.split(".")[-1]], 4.0 * g) for n, g in figures(rounded, plain).items()}


def assert_within(what, got, rounded, plain):
    """-> the worst figure / bound; prints every figure before it asserts"""
    fig, bnd = figures(got, rounded), bounds(rounded, plain)
    print(f"{what}: " + ", ".join(f"{n} {fig[n]:.2e} / {bnd[n]:.2e}" for n in fig))
    bad = {n: (fig[n], bnd[n]) for n in fig if not fig[n] <= bnd[n]}
    assert not bad, (what, bad)
    worst = max(fig[n] / bnd[n] for n in fig)
    print(f"{what}: worst figure / bound {worst:.3f}")
    return worst


# ---------------------------------------------------------------------------------------------- the cases (B = 2)
def _case(seed, spec_of, H, W, c1, c2):
    g = torch.Generator().manual_seed(seed)
    spec = spec_of(g)
    return spec, torch.randn(2, H, W, c1, generator=g).to(torch.bfloat16), DR._grad_in(g, 2, H, W, c2)


CASES = {
    "bottleneck": lambda: _case(101, lambda g: make_bottleneck(g, 16, 8), 8, 8, 16, 16),
    "c3k": lambda: _case(102, lambda g: make_c3k(g, 32, 32, 2), 8, 8, 32, 32),
    "c3k2_n1": lambda: _case(103, lambda g: make_c3k2(g, 32, 64, 1, False, 0.25), 8, 8, 32, 64),   # model.2 of yolo11n
    "c3k2_n2": lambda: _case(104, lambda g: make_c3k2(g, 32, 64, 2, False, 0.25), 8, 8, 32, 64),
    "c3k2_c3k": lambda: _case(105, lambda g: make_c3k2(g, 64, 64, 1, True, 0.5), 4, 4, 64, 64),
    "c2psa": lambda: _case(106, lambda g: make_c2psa(g, 128, 1), 4, 4, 128, 128),
}
