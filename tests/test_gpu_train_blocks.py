"""f1, the composite blocks of the trunk in training mode (obb_chanwin_bf16 of csrc/routegrad.hip; `train.Bottleneck` / `C3k` / `C3k2` / `C2PSA`):
the channel-window kernel bit for bit against torch slicing, its refusals, every block bit for bit against the same computation composed from the
existing modules with torch slicing, every block against the independent autograd restatement of tests/block_ref.py under max(FLOOR, 4 x grain)
(which test_train_blocks_cpu.py shows to separate a correct stand-in from seven wiring mistakes), the step checks of train_steps_ref.py, fold(),
and Attention.forward unchanged by the move of its v slice to the kernel.

Measured (MI355X), worst figure / bound per block against the restatement: see DESIGN.md section 3.4.1."""
import ctypes

import pytest
import torch

import attn_ref as AR
import block_ref as BR
import train_steps_ref as TS
from bounds import Guarded

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _ops():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    return ops


def _tr():
    _ops()
    import oriented_object_detection_amd.train as TR
    return TR


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rand(g, *shape):
    return (torch.randn(*shape, generator=g) * 3).to(BF)


def _pattern(*shape):
    """a recognisable finite fill: untouched channels must still hold it"""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n) % 251).float() - 125.0).reshape(shape).to(BF)


def _run_window(src, s0, n, Cd, d0, add=None, a0=0):
    """the registered op into a Guarded, pre-filled dst -> (device result, reference), both whole dst tensors on the CPU"""
    fill = _pattern(*src.shape[:-1], Cd)
    g = Guarded((*src.shape[:-1], Cd), BF, init=fill.cuda())
    torch.ops.obbhip.chanwin(src.cuda(), s0, None if add is None else add.cuda(), a0, n, g.out, d0)
    torch.cuda.synchronize()
    assert g.guards_intact(), "write outside dst"
    return g.out.cpu(), BR.chanwin_ref(src, s0, n, dst=fill, d0=d0, add=add, a0=a0)


# ---------------------------------------------------------------------------------------------- the kernel, bit for bit
@pytest.mark.parametrize("npix_shape,Cs,s0,n,Cd,d0,Ca,a0", [
    ((5,), 16, 8, 8, 8, 0, None, 0),            # the split of a single chunk
    ((2, 7, 7), 16, 0, 16, 48, 32, None, 0),    # a member into a concat
    ((2, 7, 7), 48, 16, 16, 16, 0, 16, 0),      # window + dense add into dense
    ((3, 5), 48, 32, 16, 40, 8, 32, 16),        # window + window add into a window
    ((1,), 8, 0, 8, 8, 0, 8, 0),                # one chunk in all
    ((300, 7), 24, 8, 16, 24, 0, None, 0),      # more than one workgroup, n / 8 = 2
])
def test_chanwin_matches_slicing_bit_for_bit(npix_shape, Cs, s0, n, Cd, d0, Ca, a0):
    _ops()
    g = torch.Generator().manual_seed(Cs * 100 + n + d0)
    src = _rand(g, *npix_shape, Cs)
    add = None if Ca is None else _rand(g, *npix_shape, Ca)
    got, want = _run_window(src, s0, n, Cd, d0, add, a0)
    assert torch.equal(_bits(got), _bits(want))


def test_chanwin_wrapper_allocates_and_checks():
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    src, add = _rand(g, 2, 3, 4, 32), _rand(g, 2, 3, 4, 16)
    out = ops.chanwin_bf16(src.cuda(), 8, 16)
    assert tuple(out.shape) == (2, 3, 4, 16) and out.is_contiguous()
    assert torch.equal(_bits(out.cpu()), _bits(BR.chanwin_ref(src, 8, 16)))
    out = ops.chanwin_bf16(src.cuda(), 16, 16, add=add.cuda())
    assert torch.equal(_bits(out.cpu()), _bits(BR.chanwin_ref(src, 16, 16, add=add)))
    dst = _pattern(2, 3, 4, 24)
    d = dst.cuda()
    assert ops.chanwin_bf16(src.cuda(), 0, 8, dst=d, d0=16, add=add.cuda(), a0=8) is d
    assert torch.equal(_bits(d.cpu()), _bits(BR.chanwin_ref(src, 0, 8, dst=dst, d0=16, add=add, a0=8)))
    z = lambda *s: torch.zeros(*s, dtype=BF, device="cuda")
    with pytest.raises(ValueError, match="leading dims"):
        ops.chanwin_bf16(z(2, 3, 16), 0, 8, dst=z(2, 4, 16))
    with pytest.raises(ValueError, match="leading dims"):
        ops.chanwin_bf16(z(2, 3, 16), 0, 8, add=z(3, 2, 16))
    with pytest.raises(ValueError, match="d0"):
        ops.chanwin_bf16(z(2, 3, 16), 0, 8, d0=8)
    with pytest.raises(ValueError, match="contiguous"):
        ops.chanwin_bf16(z(2, 3, 16)[..., 8:], 0, 8)


def _specials():
    """bf16 bit patterns: +-0, +-inf, NaNs with different payloads and signs, subnormals, the largest finite values, ordinary values"""
    pats = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81, 0x7FFF, 0xFFA5, 0x0001, 0x8001, 0x007F, 0x807F, 0x7F7F, 0xFF7F, 0x3F80, 0xBF80, 0x4049,
            0x0080, 0x8080, 0x3F81, 0xC2F7, 0x1234, 0x9ABC]
    return torch.tensor([p - 65536 if p >= 32768 else p for p in pats], dtype=torch.int16)


def test_chanwin_special_values():
    """Copy form: every bit pattern survives (NaN payloads, -0, subnormals).  Add form: exact on the finite results, NaN where the reference has
    NaN (inf - inf, NaN + x), infinities alike."""
    _ops()
    sp = _specials()
    k = sp.numel()
    # every pattern next to every pattern: src[p, j] = sp[p], add[p, j] = sp[j mod k]
    src = sp.view(k, 1).expand(k, 32).contiguous().view(BF)
    add = sp.repeat(2)[:32].view(1, 32).expand(k, 32).contiguous().view(BF)
    got, want = _run_window(src, 8, 24, 32, 0)
    assert torch.equal(_bits(got), _bits(want)), "the copy form changed a bit pattern"
    got, want = _run_window(src, 0, 32, 32, 0, add, 0)
    nan = torch.isnan(want.float())
    assert bool(nan.any()) and bool((~nan).any())
    assert torch.equal(torch.isnan(got.float()), nan), "NaN where the reference has none, or the reverse"
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), "the add form is not exact on the non-NaN results"


def test_chanwin_second_grid_stride_step():
    """npix * n / 8 = 21632 * 64 chunks > 4096 * 256: the grid-stride loop takes a second step.  Compared on the device against torch's own slice."""
    ops = _ops()
    npix, Cs, s0, n = 2 * 104 * 104, 520, 8, 512
    assert npix * (n // 8) > 4096 * 256
    src = torch.randint(-32768, 32767, (2, 104, 104, Cs), dtype=torch.int16, device="cuda").view(BF)
    out = ops.chanwin_bf16(src, s0, n)
    assert torch.equal(_bits(out), _bits(src[..., s0:s0 + n]))
    src.view(torch.int16).bitwise_and_(0x7F7F).bitwise_or_(0x2000)  # finite, same-sign values for the add form
    add = src[..., :n].contiguous()
    out = ops.chanwin_bf16(src, s0, n, add=add)
    assert torch.equal(_bits(out), _bits((src[..., s0:s0 + n].float() + add.float()).to(BF)))


def test_chanwin_refusals_leave_the_output_alone():
    ops = _ops()
    from oriented_object_detection_amd import _lib
    c, P, S = ops.ctx(), ops._p, ops._stream
    npix = 6
    src = torch.ones(npix, 32, dtype=BF, device="cuda")
    add = torch.ones(npix, 32, dtype=BF, device="cuda")
    fill = _pattern(npix, 32)
    g = Guarded((npix, 32), BF, init=fill.cuda())
    raw0 = g.raw.clone()
    ok = dict(src=P(src), Cs=32, s0=8, add=P(add), Ca=32, a0=8, npix=npix, n=16, dst=P(g.out), Cd=32, d0=8)

    def call(**kw):
        a = {**ok, **kw}
        ops._call("obb_chanwin_bf16", c, a["src"], a["Cs"], a["s0"], a["add"], a["Ca"], a["a0"], a["npix"], a["n"], a["dst"], a["Cd"], a["d0"], S())

    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)
    bad = [
        (dict(n=0), "n = 0"), (dict(n=12), "n = 12"), (dict(n=-8), "n = -8"),
        (dict(Cs=0), "Cs"), (dict(Cs=28), "Cs"), (dict(Cd=36), "Cd"), (dict(Cd=0), "Cd"), (dict(Ca=20), "Ca"), (dict(Ca=0), "Ca"),
        (dict(s0=4), "s0"), (dict(s0=-8), "s0"), (dict(d0=12), "d0"), (dict(d0=-8), "d0"), (dict(a0=4), "a0"), (dict(a0=-8), "a0"),
        (dict(s0=24), "runs past src"), (dict(d0=24), "runs past dst"), (dict(a0=24), "runs past add"), (dict(n=40), "runs past"),
        (dict(src=P(None)), "NULL"), (dict(dst=P(None)), "NULL"),
        (dict(src=off(src, 8)), "aligned"), (dict(add=off(add, 2)), "aligned"), (dict(dst=off(g.out, 8)), "aligned"),
        (dict(npix=0), "npix"), (dict(npix=-3), "npix"),
        (dict(src=P(g.out)), "overlaps src"), (dict(add=P(g.out)), "overlaps add"),
        (dict(src=off(g.out, 64), npix=2), "overlaps src"),   # the last of dst's two pixels is the first of src's
        (dict(add=off(g.out, -32), npix=2), "overlaps add"),
    ]
    for kw, pat in bad:
        with pytest.raises(_lib.ObbHipError, match=pat):
            call(**kw)
    torch.cuda.synchronize()
    assert torch.equal(g.raw, raw0), "a refused call wrote to its output"
    call()  # the accepted form of the same call, add NULL too
    call(add=P(None), Ca=0, a0=0)
    torch.cuda.synchronize()
    assert g.guards_intact()
    assert torch.equal(_bits(g.out.cpu()), _bits(BR.chanwin_ref(src.cpu(), 8, 16, dst=fill, d0=8)))


# ---------------------------------------------------------------------------------------------- the blocks
_CACHE = {}


def _refs(kind):
    """(case, constructor arguments on the device, plain, rounded) of a block case: the references are computed once and shared, unchanged"""
    if kind not in _CACHE:
        case = BR.CASES[kind]()
        args = BR.module_args(case[0], lambda t: t.cuda())  # the initial tensors, before the rounded run moves the running statistics
        plain = BR.run(case, True)
        rounded = BR.run(case, False)
        _CACHE[kind] = (case, args, plain, rounded)
    return _CACHE[kind]


def _device_block(TR, kind, args, groups=None):
    cls = {"bottleneck": TR.Bottleneck, "c3k": TR.C3k, "c3k2": TR.C3k2, "c2psa": TR.C2PSA}[kind]
    groups = groups or TR.ParamGroups("SGD", lr=0.01, momentum=0.9, weight_decay=5e-4)
    mod = cls(groups, *args, BR.EPS, BR.MOM)
    groups.build()
    return mod, groups


def _invs(mod):
    return {f"m.{i}.attn.qkv": m.attn.inv for i, m in enumerate(mod.m)} if hasattr(mod, "m") and hasattr(mod.m[0], "attn") else {}


class _Composed:
    """The same computation as a block of train.py, composed from the existing ConvBN / PSABlock modules with torch `[..., a:b].contiguous()`,
    torch.cat and ops.add_bf16; the leaves are registered in the block's order."""

    def __init__(self, TR, ops, kind, groups, args):
        self.ops, self.kind = ops, kind
        cb = lambda t: TR.ConvBN(groups, t[0], t[1], t[2], 1, t[3], t[4], BR.EPS, BR.MOM)
        if kind == "bottleneck":
            self.cv1, self.cv2 = cb(args[0]), cb(args[1])
        elif kind == "c3k":
            self.cv1, self.cv2, self.cv3 = cb(args[0]), cb(args[1]), cb(args[2])
            self.m = [_Composed(TR, ops, "bottleneck", groups, a) for a in args[3]]
        elif kind == "c3k2":
            self.cv1, self.cv2 = cb(args[0]), cb(args[1])
            self.m = [_Composed(TR, ops, "c3k" if args[3] else "bottleneck", groups, a) for a in args[2]]
        else:
            self.cv1, self.cv2 = cb(args[0]), cb(args[1])
            self.m = [TR.PSABlock(groups, *a, args[3], BR.EPS, BR.MOM) for a in args[2]]

    def named_blocks(self):
        own = [(n, getattr(self, n)) for n in ("cv1", "cv2", "cv3") if hasattr(self, n)]
        for i, m in enumerate(getattr(self, "m", [])):
            if isinstance(m, _Composed):
                own += [(f"m.{i}.{n}", b) for n, b in m.named_blocks()]
            else:
                own += [(f"m.{i}.{BR.PSA_NAMES[t]}", b) for t, b in (("qkv", m.attn.qkv), ("proj", m.attn.proj), ("pe", m.attn.pe), ("ffn0", m.ffn0), ("ffn1", m.ffn1))]
        return own

    def forward(self, x):
        add = self.ops.add_bf16
        if self.kind == "bottleneck":
            return add(x, self.cv2.forward(self.cv1.forward(x)))
        if self.kind == "c3k":
            a = self.cv1.forward(x)
            for m in self.m:
                a = m.forward(a)
            return self.cv3.forward(torch.cat([a, self.cv2.forward(x)], -1))
        t = self.cv1.forward(x)
        c = t.shape[-1] // 2
        if self.kind == "c3k2":
            ys = [t[..., :c].contiguous(), t[..., c:].contiguous()]
            for m in self.m:
                ys.append(m.forward(ys[-1]))
            return self.cv2.forward(torch.cat(ys, -1))
        b = t[..., c:].contiguous()
        for m in self.m:
            b = m.forward(b)
        return self.cv2.forward(torch.cat([t[..., :c].contiguous(), b], -1))

    def backward(self, dy):
        add = self.ops.add_bf16
        if self.kind == "bottleneck":
            return add(dy, self.cv1.backward(self.cv2.backward(dy)))
        if self.kind == "c3k":
            dcat = self.cv3.backward(dy)
            c_ = dcat.shape[-1] // 2
            da = dcat[..., :c_].contiguous()
            for m in reversed(self.m):
                da = m.backward(da)
            return add(self.cv1.backward(da), self.cv2.backward(dcat[..., c_:].contiguous()))
        dcat = self.cv2.backward(dy)
        n = len(self.m)
        if self.kind == "c3k2":
            c = dcat.shape[-1] // (2 + n)
            g = dcat[..., (1 + n) * c:].contiguous()
            for i in range(n, 0, -1):
                g = add(dcat[..., i * c:(i + 1) * c].contiguous(), self.m[i - 1].backward(g))
            return self.cv1.backward(torch.cat([dcat[..., :c], g], -1).contiguous())
        c = dcat.shape[-1] // 2
        db = dcat[..., c:].contiguous()
        for m in reversed(self.m):
            db = m.backward(db)
        return self.cv1.backward(torch.cat([dcat[..., :c], db], -1).contiguous())


def _base(kind):
    return "c3k2" if kind.startswith("c3k2") else kind


@pytest.mark.parametrize("kind", list(BR.CASES))
def test_block_equals_its_composition_bit_for_bit(kind):
    """out, dx, every parameter gradient and both running statistics, over an identical second ParamGroups: the window kernel copies bits and its
    add is add_bf16's fp32 add with one rounding, so nothing may differ."""
    ops, TR = _ops(), _tr()
    (spec, x, dy), args, _, _ = _refs(kind)
    mod, _ = _device_block(TR, _base(kind), args)
    g2 = TR.ParamGroups("SGD", lr=0.01, momentum=0.9, weight_decay=5e-4)
    comp = _Composed(TR, ops, _base(kind), g2, args)
    g2.build()
    assert [n for n, _ in mod.named_blocks()] == [n for n, _ in comp.named_blocks()] == [n for n, _ in BR.leaves(spec)]
    xd, dyd = x.cuda(), dy.cuda()
    got = BR.collect(mod, mod.forward(xd), mod.backward(dyd))
    want = BR.collect(comp, comp.forward(xd), comp.backward(dyd))
    torch.cuda.synchronize()
    assert set(got) == set(want)
    for n in want:
        assert torch.equal(got[n], want[n]), f"{kind}: {n} differs from the composition"
        assert bool(torch.isfinite(got[n]).all()), n


@pytest.mark.parametrize("kind", list(BR.CASES))
def test_block_against_the_autograd_restatement(kind):
    """max |got - ref| / max |ref| per quantity against the fp32 restatement at the device's rounding points, within max(FLOOR, 4 x grain), grain
    from the two references alone (block_ref's docstring).  Then fold(): the checkpoint's relative names, per-channel values against the
    restatement's leaves folded from the device's parameters and running statistics."""
    TR = _tr()
    (spec, x, dy), args, plain, rounded = _refs(kind)
    mod, _ = _device_block(TR, _base(kind), args)
    got = BR.collect(mod, mod.forward(x.cuda()), mod.backward(dy.cuda()), _invs(mod))
    torch.cuda.synchronize()
    BR.assert_within(f"{kind}", got, rounded, plain)

    folded = mod.fold()
    assert list(folded) == [n for n, _ in BR.leaves(spec)]
    invs = _invs(mod)
    for n, d in mod.named_blocks():
        f = d.gamma / torch.sqrt(d.running_var + BR.EPS)
        wf, bf = d.w * f.view(-1, 1, 1, 1), d.beta - d.running_mean * f
        if n in invs:
            wf, bf = wf[invs[n]], bf[invs[n]]
        w, b = folded[n]
        assert w.shape == wf.shape and float((w - wf).abs().flatten(1).amax(1).max()) <= TS.FOLD_TOL * float(wf.abs().max()), n
        assert float((b - bf).abs().max()) <= TS.FOLD_TOL * max(1.0, float(bf.abs().max())), n


# ---------------------------------------------------------------------------------------------- the step checks of train_steps_ref.py
@pytest.fixture(scope="module")
def env():
    TR, ops = _tr(), _ops()

    def fold_forward(mod, x):
        wf, bf = mod.fold()
        y = ops.conv_fwd_bf16(x, ops.conv_pack_bf16(wf.contiguous(), x.shape[1], x.shape[2], stride=mod.s), bf.contiguous(), mod.c2, mod.k, stride=mod.s)
        return ops.silu_bf16(y) if mod.act else y

    return TS.Env(TR, lambda t: t.cuda(), fold_forward)


def _builder(kind):
    import types

    def build(env, groups, opt):
        spec, x0, dy0 = BR.CASES[kind]()
        for _, leaf in BR.leaves(spec):
            if isinstance(leaf, BR.RefConvBN):  # what attn_ref.fold_ref reads
                leaf.seq = [types.SimpleNamespace(weight=leaf.w), leaf.bn]
        mod = BR.build_module(env.TR, groups, spec, env.dev)
        invs = _invs(mod)
        dev = dict(mod.named_blocks())
        blocks = [(n + ".", dev[n], leaf, invs.get(n)) for n, leaf in BR.leaves(spec)]
        assert list(dev) == [n for n, _ in BR.leaves(spec)]
        state = {}

        def run_ref(inp, rounded_):
            res = BR.run((spec, inp[0], inp[1]), not rounded_)
            if not rounded_:
                state["plain"] = res
            else:  # the block tests' bound, from the two references of THIS step
                built.tol = BR.bounds(res, state["plain"])
            return res

        shape_x, shape_dy = tuple(x0.shape), tuple(dy0.shape)
        built = TS.Built(env, kind, mod, blocks, lambda g: (TS._x(g, *shape_x), TS.DR._grad_in(g, *shape_dy)), run_ref,
                         fold=lambda: {n + ".": v for n, v in mod.fold().items()})
        return built
    return build


@pytest.mark.parametrize("kind", list(BR.CASES))
def test_step_checks(env, kind):
    """Gradients written, not added, NaN dummies on either side untouched; backward uses the latest forward bit for bit; three re-synchronised
    SGD-Nesterov steps under the block tests' bound with the parameters against torch.optim; fold() after the parameters have moved."""
    TS.check_grads_written(env, _builder(kind))
    TS.check_latest_forward(env, _builder(kind))
    b, worst, inp = TS.check_three_steps(env, _builder(kind), "SGD")
    TS.check_fold(b, inp[0])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- Attention unchanged
def test_attention_forward_is_unchanged_by_the_window_kernel():
    """Attention.forward with v taken by ops.chanwin_bf16 against the expression it replaces, qkv[..., nh * 64:].contiguous(), composed here from
    the block's own leaves: bit-identical output."""
    ops, TR = _ops(), _tr()
    _, nh, ref, x, _ = AR.block_case("attn", 2, 4, 4, 128)
    args = [tuple(t.clone().cuda() for t in ref[t].init) for t in AR.ATTN_TAGS]
    outs = []
    for old in (False, True):
        grp = TR.ParamGroups()
        att = TR.Attention(grp, *args, nh, BR.EPS, BR.MOM)
        grp.build()
        if not old:
            outs.append(att.forward(x.cuda()))
            continue
        qkv = att.qkv.forward(x.cuda())
        out, _ = ops.attn_fwd_bf16(qkv, nh)
        v = qkv[..., nh * 64:].contiguous()
        assert torch.equal(_bits(ops.chanwin_bf16(qkv, nh * 64, nh * 64)), _bits(v))
        outs.append(att.proj.forward(ops.add_bf16(out, att.pe.forward(v))))
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
