"""CPU side of the whole-network tests (train.Trunk / train.Net) -- not the product, nothing here touches the GPU.

  conv_table(scale, nc, ch)       the conv layers of YOLO11-OBB by Ultralytics state-dict name (oracle.yolo11_obb's channel arithmetic, no weights)
  make_state(scale, nc, ch, seed) a synthetic TRAINING state dict under those names: conv weights, BatchNorm gamma / beta / running statistics
                                  that are not the identity, the head's plain convs with bias
  state_of_oracle(model)          the state dict whose fold() is exactly the oracle model's folded (w, b)
  dense_layers(scale, nc, ch, H, W)  every dense conv (the layers ConvBN / BoxOut pack) with its INPUT map at H x W tiles
  WIRING                          the yaml graph as data: per top-level module where its input comes from
  module_input(i, outs, wiring)   what the yaml graph feeds module i, built from the modules' outputs with torch cat and nearest upsample (NHWC)
  eval_forward(folded, tiles, nc, wiring)   the eval-mode forward in fp64 on folded weights, written from WIRING and torch.nn.functional alone: an
                                  independent statement of the graph to hold against oracle.yolo11_obb.Yolo11OBB.forward_raw
  check_wiring / check_head_wiring(taps)    the bit-for-bit wiring checks on train.Trunk's / Net's / DetectHead's taps; StandInTrunk / StandInHead
                                  produce taps of the same format on the CPU, with planted mistakes
  module_spec / run_module / module_refs    the trunk's modules restated from the block_ref / route_ref / attn_ref / dw_ref leaves
  head_spec / run_branch / branch_refs / collect_branch    the nine branches of model.23 from the state dict (dw_ref.RefBlock, narrow_ref.RefHead)
"""
import math

import torch
import torch.nn.functional as F

from oracle.yolo11_obb import Yolo11OBB

# module -> ("seq", src) | ("upcat", a, b): cat(upsample2(a), b) | ("cat", a, b); the head reads HEAD_FROM
WIRING = {i: ("seq", i - 1) for i in range(1, 11)}
WIRING.update({12: ("upcat", 10, 6), 13: ("seq", 12), 15: ("upcat", 13, 4), 16: ("seq", 15), 17: ("seq", 16), 18: ("cat", 17, 13), 19: ("seq", 18),
               20: ("seq", 19), 21: ("cat", 20, 10), 22: ("seq", 21)})
HEAD_FROM = (16, 19, 22)
ORDER = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 16, 17, 18, 19, 20, 21, 22]
# fan-out tensor -> (the consumer whose gradient is summed FIRST, the one summed SECOND); 23 = the head
FAN = {19: (23, 20), 16: (23, 17), 13: (18, 15), 10: (21, 12), 6: (12, 7), 4: (15, 5)}
IN_LEVEL = {0: 1, 1: 2, 2: 4, 3: 4, 4: 8, 5: 8, 6: 16, 7: 16, 8: 32, 9: 32, 10: 32, 13: 16, 16: 8, 17: 8, 19: 16, 20: 16, 22: 32}


def conv_table(scale="n", nc=12, ch=3):
    m = Yolo11OBB.__new__(Yolo11OBB)
    m.scale, m.nc, m.ch = scale, nc, ch
    from oracle.yolo11_obb import SCALES
    m.depth, m.width, m.max_ch = SCALES[scale]
    m.convs = {}
    m._define()
    return m.convs


def is_plain(name):
    return name.startswith("model.23.") and name.endswith(".2")


def make_state(scale="n", nc=12, ch=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    st = {}
    for name, r in conv_table(scale, nc, ch).items():
        fan_in = (r.c1 // r.g) * r.k * r.k
        w = torch.randn((r.c2, r.c1 // r.g, r.k, r.k), generator=g) * ((1.0 if is_plain(name) else 1.676) / math.sqrt(fan_in))
        if is_plain(name):
            st[name + ".weight"] = w
            st[name + ".bias"] = torch.randn(r.c2, generator=g) * 0.05 + (1.0 if ".cv2." in name else -2.0 if ".cv3." in name else 0.0)
            continue
        st[name + ".conv.weight"] = w
        st[name + ".bn.weight"] = 0.75 + 0.5 * torch.rand(r.c2, generator=g)
        st[name + ".bn.bias"] = 0.1 * torch.randn(r.c2, generator=g)
        st[name + ".bn.running_mean"] = 0.1 * torch.randn(r.c2, generator=g)
        st[name + ".bn.running_var"] = 0.75 + 0.5 * torch.rand(r.c2, generator=g)
    return st


def state_of_oracle(model, eps=1e-3):
    st = {}
    for name, r in model.convs.items():
        if is_plain(name):
            st[name + ".weight"], st[name + ".bias"] = r.w.clone(), r.b.clone()
            continue
        st[name + ".conv.weight"] = r.w.clone()
        st[name + ".bn.weight"] = torch.ones(r.c2)
        st[name + ".bn.bias"] = r.b.clone()
        st[name + ".bn.running_mean"] = torch.zeros(r.c2)
        st[name + ".bn.running_var"] = torch.full((r.c2,), 1.0 - eps)  # gamma / sqrt(var + eps) = 1 up to fp32 rounding of the sum
    return st


def dense_layers(scale, nc, ch, H, W):
    """[(name, cout, cin, k, s, Hin, Win)] of every conv on the dense training kernels (groups 1, both channel counts multiples of 8)"""
    out = []
    for name, r in conv_table(scale, nc, ch).items():
        if r.g != 1 or r.c1 % 8 or r.c2 % 8:
            continue
        li = int(name.split(".")[1])
        lv = (8, 16, 32)[int(name.split(".")[3])] if li == 23 else IN_LEVEL[li]
        out.append((name, r.c2, r.c1, r.k, r.s, H // lv, W // lv))
    return out


def up2(t):
    """nearest x2 of an NHWC tensor"""
    return t.repeat_interleave(2, 1).repeat_interleave(2, 2)


def module_input(i, outs, wiring=WIRING):
    w = wiring[i]
    if w[0] == "seq":
        return outs[w[1]]
    a, b = outs[w[1]], outs[w[2]]
    return torch.cat([up2(a) if w[0] == "upcat" else a, b], -1)


# ---------------------------------------------------------------------------------------------- eval-mode forward, fp64, NCHW inside
def _conv(fold, name, x, act=True, s=1, g=1):
    w, b = fold[name]
    y = F.conv2d(x, w.double(), b.double(), stride=s, padding=w.shape[-1] // 2, groups=g)
    return y * torch.sigmoid(y) if act else y


def _bneck(fold, p, x):
    return x + _conv(fold, p + ".cv2", _conv(fold, p + ".cv1", x))


def _c3k(fold, p, x):
    a, n = _conv(fold, p + ".cv1", x), 0
    while f"{p}.m.{n}.cv1" in fold:
        a, n = _bneck(fold, f"{p}.m.{n}", a), n + 1
    return _conv(fold, p + ".cv3", torch.cat([a, _conv(fold, p + ".cv2", x)], 1))


def _c3k2(fold, p, x):
    y, n = list(_conv(fold, p + ".cv1", x).chunk(2, 1)), 0
    while f"{p}.m.{n}.cv1" in fold:
        q = f"{p}.m.{n}"
        y.append(_c3k(fold, q, y[-1]) if q + ".cv3" in fold else _bneck(fold, q, y[-1]))
        n += 1
    return _conv(fold, p + ".cv2", torch.cat(y, 1))


def _sppf(fold, p, x):
    y = [_conv(fold, p + ".cv1", x)]
    for _ in range(3):
        y.append(F.max_pool2d(y[-1], 5, 1, 2))
    return _conv(fold, p + ".cv2", torch.cat(y, 1))


def _c2psa(fold, p, x):
    t = _conv(fold, p + ".cv1", x)
    c = t.shape[1] // 2
    a, b, n = t[:, :c], t[:, c:], 0
    while f"{p}.m.{n}.attn.qkv" in fold:
        q = f"{p}.m.{n}"
        B, C, H, W = b.shape
        nh, N = C // 64, H * W
        qkv = _conv(fold, q + ".attn.qkv", b, act=False).view(B, nh, 128, N)
        qq, kk, vv = qkv[:, :, :32], qkv[:, :, 32:64], qkv[:, :, 64:]
        att = ((qq.transpose(-2, -1) @ kk) * 32 ** -0.5).softmax(-1)
        o = (vv @ att.transpose(-2, -1)).reshape(B, C, H, W) + _conv(fold, q + ".attn.pe", vv.reshape(B, C, H, W), act=False, g=C)
        b = b + _conv(fold, q + ".attn.proj", o, act=False)
        b = b + _conv(fold, q + ".ffn.1", _conv(fold, q + ".ffn.0", b), act=False)
        n += 1
    return _conv(fold, p + ".cv2", torch.cat([a, b], 1))


def eval_forward(fold, tiles, nc, wiring=WIRING, head_from=HEAD_FROM):
    """fold: {name: (w, b)}; tiles uint8 [B,H,W,ch] -> raw head [B, A, 64 + nc + 1] fp64 (forward_raw's layout); ch == 3: BGR -> RGB first"""
    x = torch.as_tensor(tiles)
    if x.shape[-1] == 3:
        x = x.flip(-1)
    x = (x.permute(0, 3, 1, 2).float() / 255.0).double()  # (the network input is the fp32 quotient, as in forward_raw)
    outs = {}
    for i in ORDER:
        if i == 0:
            outs[0] = _conv(fold, "model.0", x, s=2)
            continue
        w = wiring[i]
        if w[0] != "seq":
            a, b = outs[w[1]], outs[w[2]]
            outs[i] = torch.cat([a.repeat_interleave(2, 2).repeat_interleave(2, 3) if w[0] == "upcat" else a, b], 1)
            continue
        xin, p = outs[w[1]], f"model.{i}"
        if i in (1, 3, 5, 7, 17, 20):
            outs[i] = _conv(fold, p, xin, s=2)
        elif i == 9:
            outs[i] = _sppf(fold, p, xin)
        elif i == 10:
            outs[i] = _c2psa(fold, p, xin)
        else:
            outs[i] = _c3k2(fold, p, xin)
    res = []
    for lv, src in enumerate(head_from):
        f = outs[src]
        p = f"model.23.cv2.{lv}"
        box = _conv(fold, p + ".2", _conv(fold, p + ".1", _conv(fold, p + ".0", f)), act=False)
        p = f"model.23.cv3.{lv}"
        t = _conv(fold, p + ".0.1", _conv(fold, p + ".0.0", f, g=f.shape[1]))
        t = _conv(fold, p + ".1.1", _conv(fold, p + ".1.0", t, g=t.shape[1]))
        cls = _conv(fold, p + ".2", t, act=False)
        p = f"model.23.cv4.{lv}"
        ang = _conv(fold, p + ".2", _conv(fold, p + ".1", _conv(fold, p + ".0", f)), act=False)
        res.append(torch.cat([box, cls, ang], 1).flatten(2))
    return torch.cat(res, 2).transpose(1, 2).contiguous()


# ============================================================================================== the wiring check on `taps` (device or stand-in)
def _same(a, b):
    v = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(v(a), v(b))


def _din_slot(taps, consumer, t):
    """the gradient consumer `consumer` returned for its input tensor t"""
    if consumer == 23:
        return taps[23]["din"][HEAD_FROM.index(t)]
    w = WIRING[consumer]
    if w[0] == "seq":
        return taps[consumer]["din"]
    return taps[consumer]["din"][0 if w[1] == t else 1]


def _add(a, b):
    return (a.float() + b.float()).to(torch.bfloat16)


def check_head_wiring(taps, received=True):
    """AssertionError unless the head's gradient sum in taps[23] (train.DetectHead's tap keys) is, per level and bit for bit, partial = bf16(fp32(dx_box)
    + fp32(dx_cls)) and din = bf16(fp32(partial) + fp32(dx_angle)); received: din is also the tensor the trunk took in -- the FIRST summand of the
    fan-outs 16 and 19, model.22's dout (not for a head driven on its own)."""
    h = taps[23]
    assert len(h["branch_din"]) == len(h["partial"]) == len(h["din"]) == 3
    for lv, t in enumerate(HEAD_FROM):
        dxb, dxc, dxa = h["branch_din"][lv]
        assert _same(h["partial"][lv], _add(dxb, dxc)), f"head level {lv}: the partial sum is not bf16(box + cls)"
        assert _same(h["din"][lv], _add(h["partial"][lv], dxa)), f"head level {lv}: the sum is not bf16((box + cls) + angle)"
        if received:
            got = taps["fan"][t][0] if t in FAN else taps[t]["dout"]
            assert _same(got, h["din"][lv]), f"head level {lv}: model.{t} did not receive the head's sum"


def check_wiring(taps):
    """AssertionError unless `taps` (train.Trunk's / Net's format, taps[23] = {"in": [P3, P4, P5], "din": [d3, d4, d5]}) is the yaml graph bit for
    bit: every module's input is built from the tapped outputs (torch cat, nearest upsample), the concats hand their gradient halves back (the
    upsampled half as the fp32 sum of its 2 x 2 pixels, one rounding), a tensor with one consumer receives that consumer's gradient, and each of
    the six fan-out tensors receives bf16(fp32(first) + fp32(second)) of its two consumers' gradients in FAN's order.  Where taps[23] carries the
    head's own keys ("branch_din", "partial") the head's sum is checked too (check_head_wiring)."""
    if "branch_din" in taps[23]:
        check_head_wiring(taps)
    consumers = {i: [] for i in ORDER}
    for c, w in WIRING.items():
        for t in w[1:]:
            consumers[t].append(c)
    for t in HEAD_FROM:
        consumers[t].append(23)
    outs = {i: taps[i]["out"] for i in ORDER}
    for i in ORDER[1:]:
        w = WIRING[i]
        if w[0] == "seq":
            assert _same(taps[i]["in"], outs[w[1]]), f"model.{i}: input is not model.{w[1]}'s output"
        else:
            a, b = taps[i]["in"]
            assert _same(a, outs[w[1]]) and _same(b, outs[w[2]]), f"model.{i}: inputs are not the outputs of models {w[1]}, {w[2]}"
            assert _same(outs[i], module_input(i, outs)), f"model.{i}: not cat(up(a), b)"
    for lv, t in enumerate(HEAD_FROM):
        assert _same(taps[23]["in"][lv], outs[t]), f"head level {lv}: input is not model.{t}'s output"
    assert set(taps["fan"]) == set(FAN)
    for t in ORDER:
        cs = consumers[t]
        if not cs:
            continue
        if t not in FAN:
            assert len(cs) == 1 and _same(taps[t]["dout"], _din_slot(taps, cs[0], t)), f"model.{t}: gradient is not model.{cs[0]}'s"
            continue
        c1, c2 = FAN[t]
        first, second, s = taps["fan"][t]
        assert set(cs) == {c1, c2}
        assert _same(first, _din_slot(taps, c1, t)), f"model.{t}: the first summand is not model.{c1}'s gradient"
        assert _same(second, _din_slot(taps, c2, t)), f"model.{t}: the second summand is not model.{c2}'s gradient"
        assert _same(s, (first.float() + second.float()).to(torch.bfloat16)), f"model.{t}: the sum is not bf16(fp32 + fp32)"
        assert _same(taps[t]["dout"], s), f"model.{t}: did not receive the summed gradient"
    for c in (12, 15, 18, 21):
        da, db = taps[c]["din"]
        d, ca = taps[c]["dout"], da.shape[-1]
        assert _same(db, d[..., ca:].contiguous()), f"model.{c}: db is not the skip half of dout"
        g = d[..., :ca].float()
        if WIRING[c][0] == "upcat":  # the four pixels of a 2 x 2 cell: exact in fp32 for bf16 summands up to the last bit -> compared to 1 bf16 ulp
            B, H, W, _ = g.shape
            g = g.reshape(B, H // 2, 2, W // 2, 2, ca).double().sum((2, 4))
            ref = g.float().to(torch.bfloat16)
            lo, hi = torch.minimum(ref.float(), da.float()), torch.maximum(ref.float(), da.float())
            assert bool((hi - lo <= 2.0 ** -7 * hi.abs().clamp_min(2.0 ** -126)).all()), f"model.{c}: da is not the 2 x 2 sum of dout's upsampled half"
        else:
            assert _same(da, g.to(torch.bfloat16).contiguous()), f"model.{c}: da is not the first half of dout"


class StandInTrunk:
    """A CPU stand-in with train.Trunk's wiring code paths restated and trivial modules (module i: a fixed per-pixel linear map and tanh, stride-2
    modules on every second pixel; bf16 in and out; the backward by autograd per module), producing `taps` in Trunk's format.  wiring: the graph it
    is wired by (a planted wrong skip); drop: a fan-out tensor whose SECOND gradient is dropped (a planted lost summand)."""
    C = {0: 8, 1: 8, 2: 8, 3: 8, 4: 16, 5: 16, 6: 16, 7: 16, 8: 16, 9: 16, 10: 16, 13: 16, 16: 8, 17: 8, 19: 16, 20: 16, 22: 16}
    S2 = (0, 1, 3, 5, 7, 17, 20)

    def __init__(self, wiring=WIRING, drop=None, seed=0):
        self.wiring, self.drop, self.g = wiring, drop, torch.Generator().manual_seed(seed)
        self.A, self.saved = {}, {}

    def _mod(self, i, x):
        xr = x.float().requires_grad_(True)
        if i not in self.A:
            self.A[i] = torch.randn(x.shape[-1], self.C[i], generator=self.g) / x.shape[-1] ** 0.5
        y = torch.tanh((xr[:, ::2, ::2] if i in self.S2 else xr) @ self.A[i])
        self.saved[i] = (xr, y)
        return y.detach().to(torch.bfloat16)

    def _mod_bwd(self, i, d):
        xr, y = self.saved[i]
        return torch.autograd.grad(y, xr, d.float())[0].to(torch.bfloat16)

    def run(self, x, d_of):
        """x bf16 [B,H,W,3]; d_of(feats) -> [d3, d4, d5], or a head's tap dict with them under "din" (StandInHead) -> taps"""
        taps, outs = {"fan": {}}, {}
        for i in ORDER:
            if i == 0:
                xin = x
            elif self.wiring[i][0] == "seq":
                xin = outs[self.wiring[i][1]]
            else:
                xin = (outs[self.wiring[i][1]], outs[self.wiring[i][2]])
            if isinstance(xin, tuple):
                outs[i] = torch.cat([up2(xin[0]) if self.wiring[i][0] == "upcat" else xin[0], xin[1]], -1)
            else:
                outs[i] = self._mod(i, xin)
            taps[i] = {"in": xin, "out": outs[i]}
        feats = [outs[t] for t in HEAD_FROM]
        d = d_of(feats)
        head, d = (d, d["din"]) if isinstance(d, dict) else ({}, d)
        taps[23] = {**head, "in": feats, "din": d}
        pend ={t: [(23, g)] for t, g in zip(HEAD_FROM, d)}   # tensor -> [(consumer, gradient)] in arrival order
        for i in reversed(ORDER):
            got = pend.get(i, [])
            if i in FAN:
                got = got[:2] if len(got) >= 2 else [got[0], (None, torch.zeros_like(got[0][1]))]  # (a wrong skip moved a consumer)
                (_, first), (_, second) = got
                if self.drop == i:
                    second = torch.zeros_like(second)
                s = (first.float() + second.float()).to(torch.bfloat16)
                taps["fan"][i] = (first, got[1][1], s)
                dout = s
            else:
                dout = got[0][1]
            if i == 0:
                taps[0].update(dout=dout, din=None)
                continue
            w = self.wiring[i]
            if w[0] == "seq":
                din = self._mod_bwd(i, dout)
                pend.setdefault(w[1], []).append((i, din))
            else:
                ca = taps[i]["in"][0].shape[-1]
                g = dout[..., :ca].float()
                if w[0] == "upcat":
                    B, H, W, _ = g.shape
                    g = g.reshape(B, H // 2, 2, W // 2, 2, ca).sum((2, 4))
                din = (g.to(torch.bfloat16).contiguous(), dout[..., ca:].contiguous())
                pend.setdefault(w[1], []).append((i, din[0]))
                pend.setdefault(w[2], []).append((i, din[1]))
            taps[i].update(dout=dout, din=din)
        return taps


class StandInHead:
    """A CPU stand-in for the gradient sum of train.DetectHead.backward in its tap format: the three branch gradients of a level are given, the
    sums are restated.  mistake at `level` (the other levels are summed correctly): "drop_angle" returns box + cls, "drop_cls" box + angle,
    "order" (box + angle) + cls."""

    def __init__(self, mistake=None, level=None):
        self.mistake, self.level = mistake, level

    def backward(self, branch_din):
        partial, din = [], []
        for lv, (b, c, a) in enumerate(branch_din):
            wrong = self.mistake if lv == self.level else None
            if wrong == "drop_angle":
                p = s = _add(b, c)
            elif wrong == "drop_cls":
                p = b
                s = _add(p, a)
            elif wrong == "order":
                p = _add(b, a)
                s = _add(p, c)
            else:
                p = _add(b, c)
                s = _add(p, a)
            partial.append(p); din.append(s)
        return {"branch_din": [tuple(t) for t in branch_din], "partial": partial, "din": din}


# ============================================================================================== training-mode restatement from the leaves
import attn_ref as AR   # noqa: E402
import block_ref as BR  # noqa: E402
import dw_ref as DR     # noqa: E402
import route_ref as RR  # noqa: E402

VACUOUS = ("attn.proj.dbeta", "attn.pe.dbeta", "ffn.1.dbeta")  # sums that cancel to zero in exact arithmetic (block_ref's docstring)
MODULES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 16, 17, 19, 20, 22]
# (scale, ch, H, W, seed) of the per-module tests.  The s seed is chosen: at its 2 x 2 P5 map a near-tie in SPPF's pools can pick another argmax in
# the rounded reference than in the plain one, which moves a whole gradient between the two references (seeds 14 and 17: bound of model.9.cv1.dW
# 1.0 and 0.56); with seed 15 the largest bound is 0.15.
MODULE_CASES = [("n", 3, 64, 64, 11), ("n", 3, 64, 96, 12), ("n", 4, 64, 64, 13), ("s", 3, 64, 64, 15)]


def _bn_of(st, name):
    return tuple(st[f"{name}.bn.{k}"].detach().cpu().float() for k in ("weight", "bias", "running_mean", "running_var"))


def _leaf(st, name, s=1):
    w = st[name + ".conv.weight"].detach().cpu().float()
    R = RR.RefConvBN(torch.Generator().manual_seed(0), w.shape[1], w.shape[0], w.shape[2], s)
    with torch.no_grad():
        R.w.copy_(w)
        for dst, src in zip((R.bn.weight, R.bn.bias, R.bn.running_mean, R.bn.running_var), _bn_of(st, name)):
            dst.copy_(src)
    return R


def _block(st, name, act):
    w = st[name + ".conv.weight"].detach().cpu().float()
    groups = w.shape[0] if w.shape[1] == 1 and w.shape[2] == 3 else 1
    B = DR.RefBlock(torch.Generator().manual_seed(0), w.shape[1] * groups, w.shape[0], w.shape[2], groups, act)
    B.init = (w.clone(),) + tuple(t.clone() for t in _bn_of(st, name))
    B.reset()
    return B


def module_spec(st, i):
    """block_ref's spec of top-level module i with the state dict's parameters in its leaves (fresh leaves on every call)"""
    p = f"model.{i}"
    bneck = lambda q: {"kind": "bottleneck", "cv1": _leaf(st, q + ".cv1"), "cv2": _leaf(st, q + ".cv2")}

    def members(q, fn):
        out = []
        while f"{q}.m.{len(out)}.cv1.conv.weight" in st:
            out.append(fn(f"{q}.m.{len(out)}"))
        return out
    c3k = lambda q: {"kind": "c3k", "cv1": _leaf(st, q + ".cv1"), "cv2": _leaf(st, q + ".cv2"), "cv3": _leaf(st, q + ".cv3"), "m": members(q, bneck)}
    if i in (0, 1, 3, 5, 7, 17, 20):
        return {"kind": "conv1", "cv1": _leaf(st, p, 2)}
    if i == 9:
        return {"kind": "sppf", "cv1": _leaf(st, p + ".cv1"), "cv2": _leaf(st, p + ".cv2")}
    if i == 10:
        blocks = []
        while f"{p}.m.{len(blocks)}.attn.qkv.conv.weight" in st:
            q = f"{p}.m.{len(blocks)}"
            blocks.append({t: _block(st, f"{q}.{BR.PSA_NAMES[t]}", t == "ffn0") for t in AR.PSA_TAGS})
        return {"kind": "c2psa", "nh": st[p + ".cv1.conv.weight"].shape[0] // 128, "cv1": _leaf(st, p + ".cv1"), "cv2": _leaf(st, p + ".cv2"), "m": blocks}
    is_c3k = f"{p}.m.0.cv3.conv.weight" in st
    return {"kind": "c3k2", "c3k": is_c3k, "cv1": _leaf(st, p + ".cv1"), "cv2": _leaf(st, p + ".cv2"), "m": members(p, c3k if is_c3k else bneck)}


class _Run(BR._Run):
    def conv1(self, sp, x):
        return self.conv(sp["cv1"], x)

    def sppf(self, sp, x):
        a1 = self.conv(sp["cv1"], x)
        if sp.get("_pin") is not None and not self.plain:  # route_ref.ref_sppf's pin: one flipped rounding of a1 would move an argmax
            a1 = a1 + (sp["_pin"] - a1).detach()
        ys = [self.G(a1)]
        for _ in range(3):
            ys.append(F.max_pool2d(ys[-1], 5, 1, 2))
        return self.conv(sp["cv2"], torch.cat(ys, 1))


def stem_input(tiles):
    """the stem's conv operand: bf16(v / 255), channel order as stored, NHWC"""
    return (torch.as_tensor(tiles).cpu().float() / 255.0).to(torch.bfloat16)


def run_module(spec, x, dy, plain):
    """block_ref.run for any top-level module kind: (spec, x bf16 NHWC, dy bf16 NHWC) -> {out, dx, <leaf>.dW / dgamma / dbeta / rmean / rvar}.
    Plain first, then rounded, on FRESH specs for each pair (the rounded run moves the RefConvBN leaves' running statistics)."""
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
    for name, leaf in BR.leaves(spec):
        if not isinstance(leaf, RR.RefConvBN):
            out.update(leaf.results(name + "."))
            continue
        t = twins[id(leaf)]
        vals = (leaf.w.grad, leaf.bn.weight.grad, leaf.bn.bias.grad, leaf.bn.running_mean, leaf.bn.running_var) if t is None else \
            (t[0].grad, t[1].grad, t[2].grad, t[3], t[4])
        out.update({f"{name}.{k}": v.detach().clone() for k, v in zip(("dW", "dgamma", "dbeta", "rmean", "rvar"), vals)})
    return out


def module_refs(st, i, x, dy, pin=None):
    """-> (rounded, plain) of module i from its own input and gradient"""
    plain = run_module(module_spec(st, i), x, dy, True)
    sp = module_spec(st, i)
    if pin is not None:
        sp["_pin"] = pin
    return run_module(sp, x, dy, False), plain


def collect_module(mod, i, out, dx):
    """the device module after forward + backward -> run_module's names"""
    nchw = lambda t: t.double().cpu().permute(0, 3, 1, 2)
    if hasattr(mod, "named_blocks"):
        invs = {f"m.{j}.attn.qkv": m.attn.inv for j, m in enumerate(mod.m)} if i == 10 else None
        got = BR.collect(mod, out, dx, invs)
    else:
        got = {"out": nchw(out)}
        for name, d in ([("cv1", mod)] if i != 9 else [("cv1", mod.cv1), ("cv2", mod.cv2)]):
            got.update({f"{name}.{k}": t.detach().clone() for k, t in (("dW", d.dw), ("dgamma", d.dgamma), ("dbeta", d.dbeta), ("rmean", d.running_mean), ("rvar", d.running_var))})
        if dx is not None:
            got["dx"] = nchw(dx)
    return got


def trunk_plain(st, tiles, d):
    """The whole trunk in ONE plain fp64 autograd graph (no rounding point; the fan-out sums are autograd's): tiles uint8 NHWC, d = [d3, d4, d5]
    bf16 NHWC -> ({"P3", "P4", "P5"} NCHW, {state-dict name + ".dW" / ".dgamma" / ".dbeta"})."""
    r = _Run(True)
    specs = {i: module_spec(st, i) for i in MODULES}
    outs = {}
    for i in ORDER:
        if i == 0:
            outs[0] = r.conv1(specs[0], stem_input(tiles).double().permute(0, 3, 1, 2))
        elif WIRING[i][0] == "seq":
            outs[i] = getattr(r, specs[i]["kind"])(specs[i], outs[WIRING[i][1]])
        else:
            a, b = outs[WIRING[i][1]], outs[WIRING[i][2]]
            outs[i] = torch.cat([a.repeat_interleave(2, 2).repeat_interleave(2, 3) if WIRING[i][0] == "upcat" else a, b], 1)
    feats = [outs[t] for t in HEAD_FROM]
    torch.autograd.backward(feats, [g.double().permute(0, 3, 1, 2) for g in d])
    grads = {}
    twins = {id(R): t for R, t in r.used}
    for i in MODULES:
        for name, leaf in BR.leaves(specs[i]):
            full = f"model.{i}" + ("" if specs[i]["kind"] == "conv1" else "." + name)
            if isinstance(leaf, RR.RefConvBN):
                t = twins[id(leaf)]
                grads.update({f"{full}.dW": t[0].grad, f"{full}.dgamma": t[1].grad, f"{full}.dbeta": t[2].grad})
            else:
                res = leaf.results("")
                grads.update({f"{full}.{k}": res[k] for k in ("dW", "dgamma", "dbeta")})
    return {f"P{3 + j}": f.detach() for j, f in enumerate(feats)}, grads


def ref_module_inputs(st, tiles):
    """{module: its input bf16 NHWC} from the ROUNDED restatement chained along WIRING (no device): what each module sees inside the net"""
    r, outs, ins = _Run(False), {}, {}
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
    for i in ORDER:
        if i == 0:
            ins[0] = stem_input(tiles)
        else:
            ins[i] = module_input(i, outs)
        if i in MODULES:
            sp = module_spec(st, i)
            for m in [m for m in sp.get("m", []) if "kind" not in m]:
                for b in m.values():
                    b.reset()
            with torch.no_grad():
                outs[i] = nhwc(getattr(r, sp["kind"])(sp, ins[i].float().permute(0, 3, 1, 2)))
        else:
            outs[i] = ins[i]
    return ins, outs


def check_module(what, got, rounded, plain):
    """block_ref.assert_within with the three vacuous dbeta quantities left out of the assertion (printed all the same) -> the worst asserted
    figure / bound"""
    fig, bnd = BR.figures(got, rounded), BR.bounds(rounded, plain)
    print(f"{what}: " + ", ".join(f"{n} {fig[n]:.2e} / {bnd[n]:.2e}" for n in fig))
    bad = {n: (fig[n], bnd[n]) for n in fig if not n.endswith(VACUOUS) and not fig[n] <= bnd[n]}
    assert not bad, (what, bad)
    return max(fig[n] / bnd[n] for n in fig if not n.endswith(VACUOUS))


# ============================================================================================== the head's nine branches from the state dict
import narrow_ref as NW  # noqa: E402

HEAD_KINDS = ("box", "cls", "angle")
HEAD_CV = {"box": "cv2", "cls": "cv3", "angle": "cv4"}
# the layers of model.23 whose shape is the same at all three levels (a level mix-up among them raises nothing): {family: names under cv?.<level>}
HEAD_SAME_SHAPE = {"cv2": ("1", "2"), "cv3": ("1.0", "1.1", "2"), "cv4": ("1", "2")}


def _plain_conv(st, name):
    w, b = (st[f"{name}.{k}"].detach().cpu().float() for k in ("weight", "bias"))
    R = NW.RefHead(torch.Generator().manual_seed(0), w.shape[1], w.shape[0])
    R.init = (w.clone(), b.clone())
    R.reset()
    return R


def head_spec(st, level):
    """{"box" | "cls" | "angle": [(name under model.23.cv?.<level>, leaf)]} of one level with the state dict's parameters in the leaves, as
    criterion_ref.head_case builds them: dw_ref.RefBlock per Conv block, narrow_ref.RefHead ("out") for the plain output conv."""
    def three(q):
        return [("0", _block(st, q + ".0", True)), ("1", _block(st, q + ".1", True)), ("out", _plain_conv(st, q + ".2"))]
    c = f"model.23.cv3.{level}"
    return {"box": three(f"model.23.cv2.{level}"), "angle": three(f"model.23.cv4.{level}"),
            "cls": [(f"{i}.{j}", _block(st, f"{c}.{i}.{j}", True)) for i in (0, 1) for j in (0, 1)] + [("out", _plain_conv(st, c + ".2"))]}


def run_branch(kind, spec, x, dy, plain):
    """One branch of head_spec's `spec` from its own input x (bf16 NHWC) and the gradient dy of its logits (NHWC: bf16 for box, fp32 for cls and
    angle) -> {out, dx, <leaf>.dW / dgamma / dbeta / rmean / rvar, out.dW, out.db}, NCHW.  plain: the nn.Module stack in fp64; else the rounding
    points of criterion_ref.run_head: the leaves' own (weights, z, a; da, dz, dx), the box logits and their gradient bf16, the class and angle
    logits fp32 with their gradient rounded to bf16 where the output conv reads it."""
    leaves = spec[kind]
    for _, m in leaves:
        m.reset()
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    a = xr
    for _, m in leaves:
        a = m(a, not plain)
    if kind == "box" and not plain:
        a = DR._GradBf16.apply(DR._q(a))
    a.backward(dy.double().permute(0, 3, 1, 2))
    out = {"out": a.detach().clone(), "dx": xr.grad.clone()}
    for name, m in leaves:
        out.update(m.results(name + "."))
    return out


def branch_refs(st, level, kind, x, dy):
    """-> (rounded, plain)"""
    spec = head_spec(st, level)
    plain = run_branch(kind, spec, x, dy, True)
    return run_branch(kind, spec, x, dy, False), plain


def collect_branch(kind, br, out, dx):
    """a branch of train.DetectHead after forward + backward -> run_branch's names (copies on the CPU), every gradient read through the layer's
    OWN view of the flat buffers"""
    nchw = lambda t: t.double().cpu().permute(0, 3, 1, 2)
    blocks = [(f"{i}.{j}", b) for i, p in enumerate(br.pairs) for j, b in enumerate((p.dw, p.pw))] if kind == "cls" else \
        [(str(i), b) for i, b in enumerate(br.blocks)]
    got = {"out": nchw(out), "dx": nchw(dx), "out.dW": br.out.dw.cpu(), "out.db": br.out.db.cpu()}
    for name, d in blocks:
        got.update({f"{name}.{k}": t.cpu() for k, t in (("dW", d.dw), ("dgamma", d.dgamma), ("dbeta", d.dbeta), ("rmean", d.running_mean), ("rvar", d.running_var))})
    return got


BACKWARD_KINDS = ("dx", "dW", "dgamma", "dbeta", "db")


def head_dense_grads(seed, maps, nc):
    """A full gradient for every logit of every level (the second drive of the head tests): maps = [(B, H, W)] per level -> (d_box bf16 on
    dw_ref._grad_in's grid, d_cls fp32 N(0, 0.1^2) -- NOT bf16 values: the output conv's backward rounds them as it loads --, d_angle fp32 on the grid)"""
    g = torch.Generator().manual_seed(seed)
    return ([DR._grad_in(g, *m, 64) for m in maps], [torch.randn(*m, nc, generator=g) * 0.1 for m in maps],
            [DR._grad_in(g, *m, 1).float() for m in maps])


def fold_of_state(st, name, running_mean=None, running_var=None, eps=1e-3):
    """(w, b) of layer `name` folded from the STATE DICT's parameters and the given running statistics, in train._BNBlock.fold's operation order"""
    if is_plain(name):
        return st[name + ".weight"], st[name + ".bias"]
    f = st[name + ".bn.weight"] / torch.sqrt(running_var + eps)
    return st[name + ".conv.weight"] * f.view(-1, 1, 1, 1), st[name + ".bn.bias"] - running_mean * f
