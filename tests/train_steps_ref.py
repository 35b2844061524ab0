"""Shared by test_gpu_train_steps.py (the device modules of train.py) and test_train_steps_cpu.py (a pure-torch stand-in with planted mistakes): what
a training step leaves behind for the NEXT one -- not the product, nothing here needs the GPU.

One `Built` per module kind pairs the module on a `ParamGroups` with the fp64 reference the single-step tests already use (dw_ref.RefBlock,
narrow_ref.RefStem / RefHead and their run_* functions, attn_ref.run_block, route_ref.ref_sppf; the two box branches chain RefBlock / RefHead
under oracle.loss.dfl_loss); nothing of those references is restated here.  `resync` copies the
module's fp32 master parameters and running statistics into the reference's `init` tensors, which every run_* restores before it evaluates, so the
reference starts each step from exactly the device's state.

The checks (the same functions in both test files):
  check_grads_written     forward + backward, clone the gradients, `poison` the flat buffers with NaN, run again: every gradient view equal to its
                          clone; 5-element dummies registered before and after the module in each group still all NaN, no NaN anywhere else
  check_latest_forward    forward(x1), forward(x2), backward(da) bit-equal to a second module after forward(x2), backward(da); a *Step class:
                          two forward_backward calls against one
  check_three_steps       three steps with fresh inputs: resync, reference, device, the module's single-step criterion on every tensor; the
                          parameters after each `groups.step()` against ONE fp32 torch.optim fed the device's gradients (its state carries over)
  check_fold              fold() against the resynchronised reference's eval-mode fold, per output channel, checkpoint channel order

Criteria, as the single-step tests state them: "2e" -- per tensor e = distance of the bf16-rounded reference from the plain one, device within 2 e
of plain (test_gpu_train_dw / _attn / _narrow: DWConvBN, ClassBranchPair, ConvBN(act=False), Attention, PSABlock, StemConvBN, HeadOut, the angle
and class branches); CONVBN_TOL, BOX_STEP_TOL, BOXBRANCH_TOL, route_ref.SPPF_MEASURED -- fixed bounds on max |d| / max |ref| against the rounded
reference (test_gpu_train_bn: ConvBN with SiLU, DetectBoxBranchStep; test_gpu_loss: BoxBranchStep; test_gpu_train_route: SPPF).

Parameter bound after step k: k x PARAM_TOL x max(1, max |p|).  fp32 torch.optim against fp64 torch.optim over the same three steps
(`optim_fp32_vs_fp64`, asserted in test_train_steps_cpu.py) measures 0.020 of that bound for SGD and 0.032 for AdamW at worst, so k times the
single-step bound holds with room and nothing is derived anew."""
import math

import torch
import torch.nn.functional as F

import types

import torch.nn as nn

import attn_ref as AR
import block_ref as BR
import dw_ref as DR
import narrow_ref as NR
import route_ref as RR
from dw_ref import _GradBf16, _q
from oracle import loss as ol

EPS, MOM = DR.EPS, DR.MOM
WD = 5e-4
LR = {"SGD": 0.01, "AdamW": 0.001}
STEPS = 3
PARAM_TOL = 2e-6      # one optimiser step against torch.optim fed the same gradients, x max(1, max |p|)
FOLD_TOL = 4e-7       # fold() against the fp64 fold of the same parameters, x max |w| (x max(1, max |b|))
FOLD_RUN_TOL = 1.2e-2  # the folded block on the inference conv kernel against the module in .eval(), max |d| / max
# train.ConvBN with SiLU against the module stack at the device's rounding points, max |d| / max |ref| (test_gpu_train_bn.py)
CONVBN_TOL = {"out": 1.2e-2, "dx": 1.2e-2, "dW": 8e-3, "dgamma": 1e-3, "dbeta": 1e-3, "rmean": 1e-5, "rvar": 1e-5}
# train.DetectBoxBranchStep against the module stack under the DFL loss (test_gpu_train_bn.py): the loss relative, the rest max |d| / max |ref|.  That
# test compares no running statistics; they are held to the 2 e criterion that the angle branch, the same ConvBN -> ConvBN -> 1x1 chain, states.
BOX_STEP_TOL = {"loss": 2e-3, "dx": 1.5e-2, "dW": 1.2e-2, "dgamma": 1.2e-2, "dbeta": 1.2e-2, "db": 1.2e-2}
# train.BoxBranchStep (BatchNorm folded) against autograd at the same rounding points (test_gpu_loss.py)
BOXBRANCH_TOL = {"loss": 2e-3, "dx": 1.2e-2, "dW": 8e-3, "db": 2e-3}
SPPF_A1_TOL = 1.2e-2  # cv1's output, which the reference's pools are pinned to (test_gpu_train_route.py: the ConvBN bound)


class Env:
    """Where the modules live: `TR` (train.py, or a stand-in namespace with the same constructors), `dev` (moves a CPU tensor there) and
    `fold_forward(mod, x)` (a folded ConvBN run as the inference engine runs it -> bf16 NHWC)."""

    def __init__(self, TR, dev, fold_forward):
        self.TR, self.dev, self.fold_forward = TR, dev, fold_forward


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) + 20260)


def _nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _dist(a, ref):
    """{name: max |a - ref| / max |ref|}"""
    assert set(a) == set(ref), set(a) ^ set(ref)
    return {n: DR.rel_dist(a[n].cpu().reshape(ref[n].shape), ref[n]) for n in ref}


def _is_bn(d):
    return hasattr(d, "dgamma")


def resync(ref, dev, inv=None):
    """The device block's fp32 master parameters (and running statistics) -> the reference block, exactly: into `ref.init`, which every run_*
    restores (fp32 -> fp64 is exact).  inv: device channel order -> checkpoint order (the qkv block of Attention)."""
    srcs = (dev.w, dev.gamma, dev.beta, dev.running_mean, dev.running_var) if _is_bn(dev) else (dev.w, dev.b)
    if not hasattr(ref, "init"):  # route_ref.RefConvBN keeps no initial copy: its live tensors are the state (fp32, exact)
        dsts = (ref.w, ref.bn.weight, ref.bn.bias, ref.bn.running_mean, ref.bn.running_var)
        with torch.no_grad():
            for dst, src in zip(dsts, srcs):
                dst.copy_(src.detach().float().cpu())
        for p in ref.params():
            p.grad = None
        return
    with torch.no_grad():
        for dst, src in zip(ref.init, srcs):
            s = src.detach()
            dst.copy_((s if inv is None else s[inv.to(s.device)]).float().cpu().reshape(dst.shape))
    ref.reset()


def poison(groups):
    """every flat gradient buffer of the groups -> NaN"""
    for o in groups.opts:
        if o.n:
            o.grad.fill_(float("nan"))


class RefBlockS(DR.RefBlock):
    """dw_ref.RefBlock (dense) with a stride: the downsampling 3x3 convs"""

    def __init__(self, g, c1, c2, k, s, act):
        super().__init__(g, c1, c2, k, 1, act)
        self.s = s
        self.seq[0].stride = (s, s)

    def _conv(self, x, w):
        return F.conv2d(x, w, stride=self.s, padding=self.k // 2)


class Built:
    """A module of train.py (or its stand-in) on its parameter groups, next to its reference.
    blocks: [(tag, device block, reference block, inv)], the leaves that own parameters, in registration order; inputs(g) -> the CPU tensors of one
    step; run_ref(inp, rounded) -> {name: tensor} (the reference's run_* on its current `init`)."""

    steps_itself = False  # a *Step class: run_dev(step=True) is mod.step(...), optimiser update included
    needs_plain = True    # some tensor is held to the 2 e criterion: the reference is also evaluated without rounding

    def __init__(self, env, name, mod, blocks, inputs, run_ref, dist=_dist, tol=None, fold=None, fold_run=None):
        self.env, self.name, self.mod, self.blocks, self.inputs, self.run_ref = env, name, mod, blocks, inputs, run_ref
        self.dist, self.tol, self._fold, self.fold_run = dist, tol, fold, fold_run
        self.groups, self.dummies = None, []

    def _named(self, bn, head):
        for tag, d, _, _ in self.blocks:
            for (suffix, k, attr) in (bn if _is_bn(d) else head):
                yield tag + suffix, k, getattr(d, attr)

    def grads(self):
        """[(name, group, view)] of every parameter gradient, device channel order"""
        return list(self._named((("dW", 0, "dw"), ("dgamma", 1, "dgamma"), ("dbeta", 2, "dbeta")), (("dW", 0, "dw"), ("db", 2, "db"))))

    def params(self):
        return list(self._named((("W", 0, "w"), ("gamma", 1, "gamma"), ("beta", 2, "beta")), (("W", 0, "w"), ("b", 2, "b"))))

    def resync(self):
        for _, d, r, inv in self.blocks:
            resync(r, d, inv)

    def forward(self, x):
        return self.mod.forward(self.env.dev(x))

    def backward(self, da):
        return self.mod.backward(self.env.dev(da))

    def collect(self, out, dx, **extra):
        """-> {name: tensor} under the reference's names, checkpoint channel order"""
        got = {"out": _nchw(out), **extra}
        if dx is not None:
            got["dx"] = _nchw(dx)
        for tag, d, _, inv in self.blocks:
            r = {"dW": d.dw, **({"dgamma": d.dgamma, "dbeta": d.dbeta, "rmean": d.running_mean, "rvar": d.running_var} if _is_bn(d) else {"db": d.db})}
            got.update({tag + n: (t if inv is None else t[inv.to(t.device)]) for n, t in r.items()})
        return got

    def run_dev(self, inp, step=False):
        out = self.forward(inp[0])
        return self.collect(out, self.backward(inp[1]))

    def fold(self):
        if self._fold is not None:
            return self._fold()
        return {tag: d.fold() for tag, d, _, _ in self.blocks if _is_bn(d)}


# ---------------------------------------------------------------------------------------------- the module kinds
def _args(env, ref):
    return tuple(env.dev(t.clone()) for t in ref.init)


def _x(g, *shape):
    return torch.randn(*shape, generator=g).to(torch.bfloat16)


def _convbn(B, H, W, c1, c2, k, s, act):
    def build(env, groups, opt):
        ref = RefBlockS(_gen(B, H, W, c1, c2, k, s, act), c1, c2, k, s, act)
        a = _args(env, ref)
        mod = env.TR.ConvBN(groups, a[0], a[1], a[2], s, a[3], a[4], EPS, MOM, act=act)
        Ho, Wo = (H + s - 1) // s, (W + s - 1) // s

        def fold_run(x):
            y = env.fold_forward(mod, env.dev(x))
            ref.seq.eval()
            with torch.no_grad():
                y_ref = ref.seq(DR._nchw(x))
            ref.seq.train()
            return DR.rel_dist(_nchw(y), y_ref)

        return Built(env, f"ConvBN k{k} s{s} {c1}->{c2}", mod, [("", mod, ref, None)], lambda g: (_x(g, B, H, W, c1), DR._grad_in(g, B, Ho, Wo, c2)),
                     lambda inp, r: DR._run([ref], [""], inp[0], inp[1], r), tol=CONVBN_TOL if act else None, fold_run=fold_run)
    return build


def _dwconvbn(B, H, W, C, act):
    def build(env, groups, opt):
        ref, _, _ = DR.dwbn_case(B, H, W, C, act)
        a = _args(env, ref)
        mod = env.TR.DWConvBN(groups, a[0], a[1], a[2], act, a[3], a[4], EPS, MOM)
        return Built(env, f"DWConvBN act {act}", mod, [("", mod, ref, None)], lambda g: (_x(g, B, H, W, C), DR._grad_in(g, B, H, W, C)),
                     lambda inp, r: DR.run_dwbn((ref, inp[0], inp[1]), r))
    return build


def _stem(B, H, W, cin, c2):
    def build(env, groups, opt):
        ref, _, _ = NR.stem_case(B, H, W, cin, c2)
        a = _args(env, ref)
        mod = env.TR.StemConvBN(groups, a[0], a[1], a[2], a[3], a[4], EPS, MOM)
        inputs = lambda g: (torch.randint(0, 256, (B, H, W, cin), generator=g, dtype=torch.uint8), DR._grad_in(g, B, (H + 1) // 2, (W + 1) // 2, c2))
        return Built(env, f"StemConvBN cin {cin}", mod, [("", mod, ref, None)], inputs, lambda inp, r: NR.run_stem((ref, inp[0], inp[1]), r))
    return build


def _head(B, H, W, c, cout):
    def build(env, groups, opt):
        ref, _, _ = NR.head_case(B, H, W, c, cout)
        mod = env.TR.HeadOut(groups, *_args(env, ref))
        inputs = lambda g: (_x(g, B, H, W, c), torch.randn(B, H, W, cout, generator=g) * 0.1)  # fp32 dy, not bf16 values: the kernel rounds them
        return Built(env, f"HeadOut {c}->{cout}", mod, [("", mod, ref, None)], inputs, lambda inp, r: NR.run_head((ref, inp[0], inp[1]), r))
    return build


def _pair(B, H, W, c1, c2):
    def build(env, groups, opt):
        rdw, rpw, _, _ = DR.pair_case(B, H, W, c1, c2)
        mod = env.TR.ClassBranchPair(groups, _args(env, rdw), _args(env, rpw), EPS, MOM)
        return Built(env, "ClassBranchPair", mod, [("dw.", mod.dw, rdw, None), ("pw.", mod.pw, rpw, None)],
                     lambda g: (_x(g, B, H, W, c1), DR._grad_in(g, B, H, W, c2)), lambda inp, r: DR.run_pair((rdw, rpw, inp[0], inp[1]), r))
    return build


def _attn(kind, B, H, W, C):
    def build(env, groups, opt):
        _, nh, ref, _, _ = AR.block_case(kind, B, H, W, C)
        tags = AR.ATTN_TAGS if kind == "attn" else AR.PSA_TAGS
        args = [_args(env, ref[t]) for t in tags]
        mod = (env.TR.Attention if kind == "attn" else env.TR.PSABlock)(groups, *args, nh, EPS, MOM)
        att = mod if kind == "attn" else mod.attn
        assert torch.equal(att.perm.cpu(), AR.qkv_perm(nh))
        dev = {"qkv": att.qkv, "proj": att.proj, "pe": att.pe, **({} if kind == "attn" else {"ffn0": mod.ffn0, "ffn1": mod.ffn1})}
        blocks = [(t + ".", dev[t], ref[t], att.inv if t == "qkv" else None) for t in tags]

        def fold():
            f = mod.fold()  # (PSABlock: keyed by checkpoint-relative names)
            return {t + ".": f[t if kind == "attn" else BR.PSA_NAMES[t]] for t in tags}

        return Built(env, "Attention" if kind == "attn" else "PSABlock", mod, blocks, lambda g: (_x(g, B, H, W, C), DR._grad_in(g, B, H, W, C)),
                     lambda inp, r: AR.run_block((kind, nh, ref, inp[0], inp[1]), r), dist=AR.block_dist,
                     fold=fold)
    return build


def _angle(B, H, W, c, c4):
    def build(env, groups, opt):
        rblocks, rhead, _, _ = NR.angle_case(B, H, W, c, c4)
        mod = env.TR.DetectAngleBranch(groups, [_args(env, b)[:3] for b in rblocks], *_args(env, rhead), eps=EPS, momentum=MOM)
        for blk, r in zip(mod.blocks, rblocks):
            blk.running_mean.copy_(r.init[3]); blk.running_var.copy_(r.init[4])
        blocks = [(f"c{i}.", d, r, None) for i, (d, r) in enumerate(zip(mod.blocks, rblocks))] + [("out.", mod.out, rhead, None)]
        return Built(env, "DetectAngleBranch", mod, blocks, lambda g: (_x(g, B, H, W, c), DR._grad_in(g, B, H, W, 1).float()),
                     lambda inp, r: NR.run_angle((rblocks, rhead, inp[0], inp[1]), r))
    return build


class _StepBuilt(Built):
    """A *Step class: inputs (x, targets..., target_scores_sum); forward_backward or step in one call, no output but the loss."""
    steps_itself = True

    def run_dev(self, inp, step=False):
        args = [self.env.dev(t) if torch.is_tensor(t) else t for t in inp]
        loss, dx = (self.mod.step if step else self.mod.forward_backward)(*args)
        got = self.collect(dx, dx, loss=loss)
        del got["out"]  # (the logits stay inside the step)
        return got


class _Leaf:
    """A conv + bias whose four tensors are properties of its owner (the 1x1 of DetectBoxBranchStep, the layers of BoxBranchStep)."""

    def __init__(self, w, b, dw, db):
        self._get = {"w": w, "b": b, "dw": dw, "db": db}

    def __getattr__(self, n):
        if n in ("w", "b", "dw", "db"):
            return self._get[n]()
        raise AttributeError(n)


class _FlatPair:
    """BoxBranchStep's two FlatOptimizers under the two methods of ParamGroups that the checks use."""

    def __init__(self, *opts):
        self.opts = list(opts)

    def step(self):
        for o in self.opts:
            o.step()


class RefConvAct(NR.RefHead):
    """nn.Conv2d(c, cout, k, padding=k // 2) with bias [-> SiLU], fp64: a layer of the box branch with BatchNorm folded.  Rounded at the device's
    points: the weights, z, a, and on the way back dx, dz, da (RefHead's reset / results)."""

    def __init__(self, g, c, cout, k, act):
        self.conv, self.k, self.act = nn.Conv2d(c, cout, k, padding=k // 2), k, act
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(cout, c, k, k, generator=g) * (1.5 / (c * k * k) ** 0.5))
            self.conv.bias.copy_(torch.randn(cout, generator=g) * 0.1)
        self.init = (self.conv.weight.detach().clone(), self.conv.bias.detach().clone())
        self.conv.double()

    def __call__(self, x, rounded):
        if not rounded:
            z = self.conv(x)
            return F.silu(z) if self.act else z
        z = _GradBf16.apply(_q(F.conv2d(_GradBf16.apply(x), _q(self.conv.weight), self.conv.bias, padding=self.k // 2)))
        return _GradBf16.apply(_q(F.silu(z))) if self.act else z


def run_dfl(layers, tags, inp, rounded, round_logits):
    """layers (RefBlock / RefHead / RefConvAct) in a chain -> 4 x 16 DFL logits -> oracle.loss.dfl_loss, backward.  round_logits: the last layer
    leaves fp64 logits (RefHead) that the device holds, with their gradient, in bf16."""
    x, tgt, wgt, tss = inp
    for b in layers:
        b.reset()
    xr = DR._nchw(x).clone().requires_grad_(True)
    a = xr
    for b in layers:
        a = b(a, rounded)
    if rounded and round_logits:
        a = _GradBf16.apply(_q(a))
    loss = ol.dfl_loss(a.permute(0, 2, 3, 1).reshape(-1, a.shape[1]), tgt.double(), wgt.double(), tss)
    loss.backward()
    out = {"loss": loss.detach().reshape(1).clone(), "dx": xr.grad.clone()}
    for b, t in zip(layers, tags):
        out.update(b.results(t))
    return out


def _dfl_inputs(B, H, W, c):
    def inputs(g):
        n = B * H * W
        tgt = torch.rand(n, 4, generator=g) * 14.5
        wgt = torch.rand(n, generator=g) * (torch.rand(n, generator=g) < 0.3)  # ~30 % foreground anchors carry a weight
        return _x(g, B, H, W, c), tgt, wgt, float(wgt.sum().clamp_min(1.0))
    return inputs


def _box_step(B, H, W, c):
    def build(env, groups, opt):
        g = _gen(B, H, W, c, 64)
        rblocks, rhead = [RefBlockS(g, c, c, 3, 1, True) for _ in range(2)], NR.RefHead(g, c, 64)
        mod = env.TR.DetectBoxBranchStep([_args(env, b)[:3] for b in rblocks], *_args(env, rhead), opt, lr=LR[opt], momentum=0.9, weight_decay=WD, eps=EPS,
                                         bn_momentum=MOM)
        for blk, r in zip(mod.blocks, rblocks):
            blk.running_mean.copy_(r.init[3]); blk.running_var.copy_(r.init[4])
        leaf = _Leaf(lambda: mod.w3, lambda: mod.b3, lambda: mod.dw3, lambda: mod.db3)
        blocks = [(f"c{i}.", d, r, None) for i, (d, r) in enumerate(zip(mod.blocks, rblocks))] + [("out.", leaf, rhead, None)]
        b = _StepBuilt(env, "DetectBoxBranchStep", mod, blocks, _dfl_inputs(B, H, W, c),
                       lambda inp, r: run_dfl(rblocks + [rhead], ["c0.", "c1.", "out."], inp, r, True), tol=BOX_STEP_TOL)
        b.groups = mod.groups
        return b
    return build


def _boxbranch_step(B, H, W, c):
    def build(env, groups, opt):
        g = _gen(B, H, W, c, 3)
        layers = [RefConvAct(g, c, c, 3, True), RefConvAct(g, c, c, 3, True), RefConvAct(g, c, 64, 1, False)]
        mod = env.TR.BoxBranchStep([env.dev(r.init[0].clone()) for r in layers], [env.dev(r.init[1].clone()) for r in layers], H, W, optimizer=opt, lr=LR[opt],
                                   momentum=0.9, weight_decay=WD)
        leaf = lambda i: _Leaf(lambda: mod.w[i], lambda: mod.b[i], lambda: mod.dw[i], lambda: mod.db[i])
        tags = [f"l{i}." for i in range(3)]
        b = _StepBuilt(env, "BoxBranchStep", mod, [(t, leaf(i), r, None) for i, (t, r) in enumerate(zip(tags, layers))], _dfl_inputs(B, H, W, c),
                       lambda inp, r: run_dfl(layers, tags, inp, r, False), tol=BOXBRANCH_TOL)
        b.groups, b.needs_plain = _FlatPair(mod.opt_w, mod.opt_b), False
        return b
    return build


class _SPPFBuilt(Built):
    """route_ref's reference is ONE evaluation (fp32 autograd at the forward rounding points) that needs the device's a1 to pin its pools to:
    run_ref follows run_dev."""
    needs_plain = False

    def run_dev(self, inp, step=False):
        got = super().run_dev(inp)
        got["a1"] = _nchw(self.mod.cat[..., :self.mod.cv1.c2])
        return got


def _sppf(B, H, W, c1, c2):
    def build(env, groups, opt):
        g = _gen(B, H, W, c1, c2, 9)
        refs = [RR.RefConvBN(g, c1, c1 // 2), RR.RefConvBN(g, 2 * c1, c2)]
        for r in refs:  # what attn_ref.fold_ref reads
            r.seq = [types.SimpleNamespace(weight=r.w), r.bn]
        dev_args = lambda r: tuple(env.dev(t.detach().clone()) for t in (r.w, r.bn.weight, r.bn.bias, r.bn.running_mean, r.bn.running_var))
        mod = env.TR.SPPF(groups, dev_args(refs[0]), dev_args(refs[1]), eps=EPS, momentum=MOM)

        def run_ref(inp, rounded):
            xr = _nchw(inp[0]).float().requires_grad_(True)
            a1, out = RR.ref_sppf(refs[0], refs[1], xr, _nchw(mod.cat[..., :c1 // 2]).float())
            out.backward(_nchw(inp[1]).float())
            res = {"out": out.detach(), "dx": xr.grad, "a1": a1.detach()}
            for t, r in zip(("cv1.", "cv2."), refs):
                res.update({t + "dW": r.w.grad, t + "dgamma": r.bn.weight.grad, t + "dbeta": r.bn.bias.grad, t + "rmean": r.bn.running_mean.clone(),
                            t + "rvar": r.bn.running_var.clone()})
            return res

        m = RR.SPPF_MEASURED[(B, H, W, c1, c2)]
        tol = {n: max(2.5 * v, RR.FLOOR[n.split(".")[-1]]) for n, v in m.items()}  # route_ref.assert_measured's bound
        tol["a1"] = SPPF_A1_TOL
        return _SPPFBuilt(env, "SPPF", mod, [("cv1.", mod.cv1, refs[0], None), ("cv2.", mod.cv2, refs[1], None)],
                          lambda g: (_x(g, B, H, W, c1), (torch.randn(B, H, W, c2, generator=g) * 0.1).to(torch.bfloat16)), run_ref, tol=tol)
    return build


def _class_step(B, H, W, c, c3, nc):
    def build(env, groups, opt):
        rpairs, rhead, _, _, _ = NR.class_case(B, H, W, c, c3, nc)
        mod = env.TR.DetectClassBranchStep([(_args(env, dw), _args(env, pw)) for dw, pw in rpairs], *_args(env, rhead), optimizer=opt, lr=LR[opt], momentum=0.9,
                                           weight_decay=WD, eps=EPS, bn_momentum=MOM)
        blocks = [(f"p{i}.{n}.", d, r, None) for i, (p, rp) in enumerate(zip(mod.pairs, rpairs)) for n, d, r in (("dw", p.dw, rp[0]), ("pw", p.pw, rp[1]))]
        blocks.append(("out.", mod.out, rhead, None))

        def inputs(g):
            t = torch.rand(B, H, W, nc, generator=g) * (torch.rand(B, H, W, nc, generator=g) < 0.1).float()  # sparse soft targets
            return _x(g, B, H, W, c), t, max(float(t.sum()), 1.0)

        b = _StepBuilt(env, "DetectClassBranchStep", mod, blocks, inputs, lambda inp, r: NR.run_class((rpairs, rhead) + tuple(inp), r))
        b.groups = mod.groups
        return b
    return build


# the smallest shapes at which the kernels still take their distinct paths, batch 2
KINDS = {
    "convbn_k3_c8": _convbn(2, 9, 9, 16, 24, 3, 1, True),       # narrow: the c8 weight-gradient route
    "convbn_k1_c64": _convbn(2, 9, 9, 64, 64, 1, 1, True),      # the c64 route
    "convbn_k3_s2": _convbn(2, 9, 9, 16, 16, 3, 2, True),       # stride 2 on an odd map
    "convbn_k1_noact": _convbn(2, 4, 4, 64, 128, 1, 1, False),
    "dwconvbn_act": _dwconvbn(2, 9, 7, 24, True),
    "dwconvbn_noact": _dwconvbn(2, 9, 7, 24, False),
    "stem_cin3": _stem(2, 18, 14, 3, 16),
    "stem_cin4": _stem(2, 18, 14, 4, 16),
    "head_12": _head(2, 5, 5, 64, 12),
    "head_1": _head(2, 5, 5, 64, 1),
    "class_pair": _pair(2, 9, 9, 64, 80),
    "attention": _attn("attn", 2, 4, 4, 128),
    "psablock": _attn("psa", 2, 4, 4, 128),
    "sppf": _sppf(2, 4, 4, 128, 128),
    "angle_branch": _angle(2, 13, 13, 64, 16),
    "class_step": _class_step(2, 13, 13, 64, 64, 12),
    "box_step": _box_step(2, 13, 13, 64),
    "boxbranch_step": _boxbranch_step(2, 13, 13, 64),   # BatchNorm folded: conv + bias + SiLU, bias_grad_bf16
}
STEP_KINDS = ["class_step", "box_step", "boxbranch_step"]
MODULE_KINDS = [k for k in KINDS if k not in STEP_KINDS]


def make(env, kind, opt="SGD", dummies=False):
    """kind: a key of KINDS or a builder (env, groups, opt) -> Built.  dummies: a 5-element tensor in each group before and after the module (a
    *Step class owns its groups: none there)."""
    build = KINDS[kind] if isinstance(kind, str) else kind
    if isinstance(kind, str) and kind in STEP_KINDS:
        return build(env, None, opt)  # (it owns its groups)
    groups = env.TR.ParamGroups(opt, lr=LR[opt], momentum=0.9, weight_decay=WD)
    dummy = lambda: [groups.add(k, env.dev(torch.zeros(5))) for k in range(3)] if dummies else []
    pre = dummy()
    b = build(env, groups, opt)
    post = dummy()
    groups.build()
    b.groups, b.dummies = groups, pre + post
    return b


# ---------------------------------------------------------------------------------------------- the checks
def check_grads_written(env, kind):
    """a. Gradients are written, not added to, and nothing outside the module's slices is written."""
    b = make(env, kind, dummies=True)
    inp = b.inputs(_gen(1))
    b.run_dev(inp)
    want = [t.clone() for _, _, t in b.grads()]
    assert all(bool(torch.isfinite(w).all()) for w in want)
    poison(b.groups)
    b.run_dev(inp)
    for (n, _, t), w in zip(b.grads(), want):
        assert torch.equal(t, w), f"{b.name}: {n} differs once the buffer held NaN before the backward: added to, or not written in full"
    for i in b.dummies:
        assert bool(torch.isnan(b.groups.grad[i]).all()), f"{b.name}: a gradient was written outside the module's slices (dummy item {i})"
    left = sum(int(torch.isnan(o.grad).sum()) for o in b.groups.opts if o.n)
    assert left == 5 * len(b.dummies), f"{b.name}: {left} NaN left in the gradient buffers, {5 * len(b.dummies)} dummy elements"


def check_latest_forward(env, kind):
    """b. forward(x1), forward(x2), backward(da) == forward(x2), backward(da) on a module built from the same initial tensors, bit for bit."""
    b1, b2 = make(env, kind), make(env, kind)
    g = _gen(2)
    if b1.steps_itself:  # forward_backward(inputs 1), forward_backward(inputs 2) against a fresh module on inputs 2 (batch statistics: the
        inp1, inp2 = b1.inputs(g), b1.inputs(g)  # running statistics, which differ, do not enter)
        b1.run_dev(inp1)
        r1, r2 = b1.run_dev(inp2), b2.run_dev(inp2)
        for n in r1:
            if not n.endswith(("rmean", "rvar")):
                assert torch.equal(r1[n], r2[n]), f"{b1.name}: {n} does not come from the latest forward"
        return
    (x1, _), (x2, da) = b1.inputs(g), b1.inputs(g)
    assert not torch.equal(x1, x2)
    b1.forward(x1)
    o1 = b1.forward(x2)
    dx1 = b1.backward(da)
    o2 = b2.forward(x2)
    dx2 = b2.backward(da)
    assert torch.equal(o1, o2), f"{b1.name}: the second forward's output depends on the first"
    assert (dx1 is None and dx2 is None) or torch.equal(dx1, dx2), f"{b1.name}: dx does not come from the latest forward"
    for (n, _, t1), (_, _, t2) in zip(b1.grads(), b2.grads()):
        assert torch.equal(t1, t2), f"{b1.name}: {n} does not come from the latest forward"


def compare(b, got, plain, rounded, what):
    """The module's single-step criterion on every tensor -> {name: figure / bound}; asserts all <= 1.  b.tol names the tensors with a fixed bound
    on max |d| / max |ref| against the rounded reference (by full name, else by the name's last part); every other tensor is held to 2 e."""
    tol = b.tol or {}
    bound_of = lambda n: tol.get(n, tol.get(n.split(".")[-1]))
    d_r = b.dist(got, rounded) if tol else {}
    names = list(d_r) if tol else None
    if plain is not None:
        d_p, e = b.dist(got, plain), b.dist(rounded, plain)
        names = list(d_p)
    ratio, shown = {}, []
    for n in names:
        t = bound_of(n)
        if t is not None:
            ratio[n] = d_r[n] / t
            shown.append(f"{n} {d_r[n]:.2e}")
        else:
            ratio[n] = d_p[n] / (2 * e[n]) if e[n] > 0 else (0.0 if d_p[n] == 0 else math.inf)
            shown.append(f"{n} {d_p[n]:.2e} (e {e[n]:.2e})")
    print(f"{what}: " + ", ".join(shown))
    bad = {n: r for n, r in ratio.items() if not r <= 1.0}
    assert not bad, (what, bad)
    return ratio


def _optim_ref(params, opt):
    groups = [{"params": [p for k, p in params if k == j], "weight_decay": WD if j == 0 else 0.0} for j in range(3)]
    groups = [g for g in groups if g["params"]]
    if opt == "SGD":
        return torch.optim.SGD(groups, lr=LR[opt], momentum=0.9, nesterov=True, foreach=False)
    return torch.optim.AdamW(groups, lr=LR[opt], betas=(0.9, 0.999), foreach=False)


def check_three_steps(env, kind, opt):
    """c / e. -> (built, worst, the last step's inputs): three steps with fresh inputs, the reference resynchronised at the start of each.  worst["tensors"] is the largest
    figure / bound of the single-step criterion, worst["params"] that of |p - torch.optim's p| / (k PARAM_TOL max(1, max |p|))."""
    b = make(env, kind, opt)
    tparams = [(k, torch.nn.Parameter(t.detach().float().cpu().clone())) for _, k, t in b.params()]
    topt = _optim_ref(tparams, opt)  # built once: momentum / Adam moments and the step count carry over
    g = _gen(3, opt == "SGD")
    worst = {"tensors": 0.0, "params": 0.0}
    for k in range(1, STEPS + 1):
        inp = b.inputs(g)
        b.resync()
        plain = b.run_ref(inp, False) if b.needs_plain else None
        got = b.run_dev(inp, step=True)  # (a *Step updates its parameters here: the reference holds the resynchronised copies)
        rounded = b.run_ref(inp, True)
        ratio = compare(b, got, plain, rounded, f"{b.name} {opt} step {k}")
        worst["tensors"] = max(worst["tensors"], max(ratio.values()))
        for (_, p), (_, _, gr) in zip(tparams, b.grads()):
            p.grad = gr.detach().float().cpu().clone().reshape(p.shape)
        topt.step()
        if not b.steps_itself:
            b.groups.step()
        for (_, p), (n, _, d) in zip(tparams, b.params()):
            err = float((d.detach().cpu() - p.detach()).abs().max())
            bound = k * PARAM_TOL * max(1.0, float(p.detach().abs().max()))
            worst["params"] = max(worst["params"], err / bound)
            assert err <= bound, (b.name, opt, k, n, err, bound)
    print(f"{b.name} {opt}: worst figure / bound {worst['tensors']:.2f}, parameters after a step {worst['params']:.3f}")
    return b, worst, inp


def check_fold(b, x):
    """d. fold() of every BatchNorm block against the eval-mode fold of the resynchronised reference, per output channel, in checkpoint channel
    order (FOLD_TOL: what the existing fold test of Attention / PSABlock asserts; those of DWConvBN and StemConvBN compare (w, b) with the formula
    and run no kernel either); a single ConvBN also runs folded through the inference conv on x against its reference module in .eval(), as its
    existing fold test does."""
    b.resync()
    folded = b.fold()
    for tag, d, r, _ in b.blocks:
        if not _is_bn(d):
            continue
        gam = r.seq[1].weight.detach()
        assert gam.unique().numel() == gam.numel()  # distinct per channel: a permuted fold cannot pass
        wf, bf = AR.fold_ref(r)
        w, bias = (t.double().cpu() for t in folded[tag])
        ew, eb = (w - wf).abs().flatten(1).amax(1), (bias - bf).abs()
        tw, tb = FOLD_TOL * float(wf.abs().max()), FOLD_TOL * max(1.0, float(bf.abs().max()))
        assert bool((ew <= tw).all()) and bool((eb <= tb).all()), \
            f"{b.name}: fold() of {tag or 'the block'} is off at output channels {sorted(set(torch.nonzero((ew > tw) | (eb > tb)).flatten().tolist()))[:8]} ..."
    if b.fold_run is not None:
        e = b.fold_run(x)
        print(f"{b.name}: folded, on the inference conv: max |d| / max {e:.2e}")
        assert e <= FOLD_RUN_TOL, (b.name, e)


def optim_fp32_vs_fp64(opt, n=4096, seed=0):
    """fp32 torch.optim against fp64 torch.optim, three groups, the same (fp32) gradients over STEPS steps -> the worst |p32 - p64| / (k PARAM_TOL
    max(1, max |p|)): what two correct implementations may differ by, as a fraction of the bound check_three_steps uses."""
    g = torch.Generator().manual_seed(seed)
    init = [(0, torch.randn(n, generator=g) * 0.2), (1, torch.rand(n, generator=g) + 0.5), (2, torch.randn(n, generator=g) * 0.2)]
    p32 = [(k, torch.nn.Parameter(t.clone())) for k, t in init]
    p64 = [(k, torch.nn.Parameter(t.double())) for k, t in init]
    o32, o64 = _optim_ref(p32, opt), _optim_ref(p64, opt)
    worst = 0.0
    for k in range(1, STEPS + 1):
        for (_, a), (_, b) in zip(p32, p64):
            a.grad = torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=g))
            b.grad = a.grad.double()
        o32.step(); o64.step()
        for (_, a), (_, b) in zip(p32, p64):
            worst = max(worst, float((a.detach().double() - b.detach()).abs().max()) / (k * PARAM_TOL * max(1.0, float(b.detach().abs().max()))))
    return worst
