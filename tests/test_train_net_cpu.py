"""train.Trunk / train.Net without a GPU: construction from an Ultralytics-named state dict, the names and the registration order, fold(), and the
wiring of the graph against the oracle's own forward (net_ref.eval_forward is written from net_ref.WIRING; oracle.yolo11_obb.Yolo11OBB.forward_raw
is an independent statement of the same graph).  No kernel runs here: the constructors only register tensors, and fold() is plain torch."""
import re

import numpy as np
import pytest
import torch

import net_ref as NR
from conftest import ROOT
from oracle.yolo11_obb import Yolo11OBB


def _train():
    import __graft_entry__ as g
    g._load_build_module().build()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import train
    return train


@pytest.fixture(scope="module")
def oracle_n():
    return Yolo11OBB("n", nc=12, ch=3, seed=3)


@pytest.mark.parametrize("scale,nc,ch", [("n", 12, 3), ("n", 12, 4), ("s", 12, 3), ("s", 5, 3)])
def test_names_and_shapes_equal_the_oracles(scale, nc, ch):
    """Net.from_state's named_blocks() = the oracle's conv keys, in the oracle's (= checkpoint) order per branch family, with the same
    (c1, c2, k, s, g); every parameter tensor of the state dict is held (value for value, the qkv rows through the device permutation)."""
    TR = _train()
    st = NR.make_state(scale, nc, ch, seed=1)
    net = TR.Net.from_state(st, scale, nc, ch)
    table = NR.conv_table(scale, nc, ch)
    blocks = net.named_blocks()
    names = [n for n, _ in blocks]
    assert len(names) == len(table) and set(names) == set(table)  # (the oracle defines the stride-2 convs before the C3k2s: its order is not the checkpoint's)
    assert [n for n in names if n.startswith("model.23.")] == [n for n in table if n.startswith("model.23.")]
    for name, b in blocks:
        r = table[name]
        k, s = getattr(b, "k", 1), getattr(b, "s", 1)
        g = b.c1 if isinstance(b, TR.DWConvBN) else 1
        assert (b.c1, b.c2, k, s, g) == (r.c1, r.c2, r.k, r.s, r.g), name
        w = st[name + (".weight" if NR.is_plain(name) else ".conv.weight")]
        if name.endswith("attn.qkv"):
            nh = r.c1 // 64
            assert torch.equal(b.w, w[TR.qkv_device_order(nh)]), name
        else:
            assert torch.equal(b.w, w), name
    assert sum(p.numel() for p in net.groups.param) == sum(v.numel() for k, v in st.items() if "running" not in k)


def test_registration_order_is_pinned():
    """Group 0 of the flat parameters holds the conv weights in checkpoint order; the first entries and the trunk / head boundary are pinned by name."""
    TR = _train()
    st = NR.make_state("n", 12, 3, seed=2)
    net = TR.Net.from_state(st, "n", 12, 3)
    names = [n for n, _ in net.named_blocks()]
    assert names[:8] == ["model.0", "model.1", "model.2.cv1", "model.2.cv2", "model.2.m.0.cv1", "model.2.m.0.cv2", "model.3", "model.4.cv1"]
    assert names[names.index("model.6.cv2") + 1:names.index("model.7")] == ["model.6.m.0.cv1", "model.6.m.0.cv2", "model.6.m.0.cv3", "model.6.m.0.m.0.cv1",
                                                                           "model.6.m.0.m.0.cv2", "model.6.m.0.m.1.cv1", "model.6.m.0.m.1.cv2"]
    assert names[names.index("model.10.cv2") + 1:names.index("model.13.cv1")] == [f"model.10.m.0.{t}" for t in ("attn.qkv", "attn.proj", "attn.pe", "ffn.0", "ffn.1")]
    head = [n for n in names if n.startswith("model.23.")]
    assert head[:4] == ["model.23.cv2.0.0", "model.23.cv2.0.1", "model.23.cv2.0.2", "model.23.cv2.1.0"] and names.index(head[0]) == len(names) - len(head)
    assert [n.split(".")[2] for n in head] == ["cv2"] * 9 + ["cv3"] * 15 + ["cv4"] * 9
    flat, off = net.groups.opts[0].param, 0
    for name, b in net.named_blocks():  # the weights lie in the flat buffer in exactly this order, back to back
        assert b.w.storage_offset() - flat.storage_offset() == off, name
        off += b.w.numel()
    assert off == flat.numel()


@pytest.mark.parametrize("scale", ["m", "l", "x", "q"])
def test_other_scales_raise(scale):
    TR = _train()
    st = NR.make_state("n", 12, 3, seed=1)
    with pytest.raises(ValueError):
        TR.Net.from_state(st, scale, 12, 3)


def test_wrong_width_or_ch_raises():
    TR = _train()
    with pytest.raises(ValueError):
        TR.Net.from_state(NR.make_state("s", 12, 3, seed=1), "n", 12, 3)
    with pytest.raises(ValueError):
        TR.Net.from_state(NR.make_state("n", 12, 4, seed=1), "n", 12, 3)


def test_fold_and_wiring_against_the_oracle(oracle_n):
    """Net.fold() of the oracle's weights gives them back (names, qkv channel order), and net_ref.eval_forward on them -- the graph of
    net_ref.WIRING -- equals the oracle's fp64 forward: two independent statements of the graph agree.  64 x 96 tiles (P5 = 2 x 3)."""
    TR = _train()
    net = TR.Net.from_state(NR.state_of_oracle(oracle_n), "n", 12, 3)
    fold = net.fold()
    assert list(fold) != [] and set(fold) == set(oracle_n.convs)
    for name, r in oracle_n.convs.items():
        w, b = fold[name]
        assert w.shape == r.w.shape and float((w - r.w).abs().max()) <= 2e-7 * float(r.w.abs().max()), name
        assert float((b - r.b).abs().max()) <= 2e-7 * max(1.0, float(r.b.abs().max())), name
    tiles = np.random.default_rng(5).integers(0, 256, (2, 64, 96, 3), dtype=np.uint8)
    ref = oracle_n.forward_raw(tiles, "fp64")
    exact = {n: (r.w, r.b) for n, r in oracle_n.convs.items()}
    got = NR.eval_forward(exact, tiles, 12)
    scale = float(ref.abs().max())
    print(f"  eval_forward vs forward_raw (fp64, same weights): max |d| / max |ref| = {float((got - ref).abs().max()) / scale:.3e}")
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-10 * scale
    got_f = NR.eval_forward(fold, tiles, 12)  # through Net.fold(): fp32 folding of gamma / sqrt(var + eps) = 1 - O(2^-24)
    assert float((got_f - ref).abs().max()) <= 1e-4 * scale
    # planted wiring mistakes in the stand-in graph must be caught by the same comparison
    for wrong in ({**NR.WIRING, 21: ("cat", 20, 9)}, {**NR.WIRING, 18: ("cat", 17, 6)}):
        bad = NR.eval_forward(exact, tiles, 12, wiring=wrong)
        assert float((bad - ref).abs().max()) > 1e-3 * scale
    bad = NR.eval_forward(exact, tiles, 12, head_from=(16, 13, 22))
    assert float((bad - ref).abs().max()) > 1e-3 * scale


def test_trunk_docstring_states_the_fan_out_order():
    """The six fan-out sums and their order (net_ref.FAN) are stated in Trunk's docstring, which the GPU wiring test checks bit for bit."""
    TR = _train()
    doc = TR.Trunk.__doc__
    for t, (first, second) in NR.FAN.items():
        assert re.search(rf"\b{t}:", doc), t
    assert "FIRST" in doc and "SECOND" in doc


def test_abi_of_the_multi_pack():
    from oriented_object_detection_amd import _lib, ops
    hdr = open(f"{ROOT}/include/obbhip.h").read()
    for name in ("obb_conv_pack_plan", "obb_conv_pack_multi_bf16"):
        m = re.search(rf"\bint {name}\(([^;]*)\);", hdr, re.S)
        assert m and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(",")), name
    assert f"#define OBB_PACK_TABLE_HEAD {_lib.PACK_TABLE_HEAD}" in hdr and f"#define OBB_PACK_TABLE_REC {_lib.PACK_TABLE_REC}" in hdr
    assert callable(ops.conv_pack_plan) and callable(ops.conv_pack_multi_bf16) and hasattr(torch.ops.obbhip, "conv_pack_multi")
    src = open(f"{ROOT}/oriented-object-detection_amd/csrc/convgrad.hip").read()
    assert src.count("pack_conv_elem(") == 3  # one definition, one call per kernel


def test_wiring_check_catches_planted_mistakes():
    """net_ref.check_wiring (the check the GPU test applies to the device's taps) passes a correct stand-in and fails one with a skip taken from
    the wrong layer and one with a fan-out gradient dropped, for every fan-out tensor."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 96, 3, generator=g).to(torch.bfloat16)
    d_of = lambda fs: [(torch.randn(f.shape, generator=g) * 0.1).to(torch.bfloat16) for f in fs]
    NR.check_wiring(NR.StandInTrunk().run(x, d_of))
    for wrong in ({**NR.WIRING, 21: ("cat", 20, 9)}, {**NR.WIRING, 18: ("cat", 17, 6)}):
        with pytest.raises(AssertionError, match="input"):
            NR.check_wiring(NR.StandInTrunk(wiring=wrong).run(x, d_of))
    for t in NR.FAN:
        with pytest.raises(AssertionError, match=rf"model\.{t}: the sum is not"):
            NR.check_wiring(NR.StandInTrunk(drop=t).run(x, d_of))


@pytest.mark.parametrize("scale,ch,H,W,seed", NR.MODULE_CASES, ids=lambda v: str(v))
def test_module_bounds_stay_below_half(scale, ch, H, W, seed):
    """The per-module bounds of test_gpu_train_net.py, max(FLOOR, 4 x grain), at the inputs the modules see inside the net, from the two
    references alone: none but the three documented vacuous dbeta quantities reaches 0.5 (a bound of 0.5 would pass a half-wrong result).  The
    gradient fed in here is seeded noise (the device test uses the net's own); the seeds are net_ref.MODULE_CASES'."""
    st = NR.make_state(scale, 12, ch, seed=seed)
    tiles = torch.randint(0, 256, (2, H, W, ch), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    ins, outs = NR.ref_module_inputs(st, tiles)
    g = torch.Generator().manual_seed(seed + 100)
    worst = {}
    for i in NR.MODULES:
        dy = NR.DR._grad_in(g, *outs[i].shape)
        rounded, plain = NR.module_refs(st, i, ins[i], dy)
        bnd = NR.BR.bounds(rounded, plain)
        for n, b in bnd.items():
            if i == 0 and n == "dx":
                continue  # (the stem's input is the image: no dx)
            if not n.endswith(NR.VACUOUS):
                worst[f"model.{i}.{n}"] = b
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("  largest bounds:", ", ".join(f"{n} {b:.3f}" for n, b in top))
    assert top[0][1] < 0.5, top


# ---------------------------------------------------------------------------------------------- the head inside the net
def _branch_dx_of(g):
    return lambda fs: [tuple((torch.randn(f.shape, generator=g) * 0.1).to(torch.bfloat16) for _ in range(3)) for f in fs]


def test_head_wiring_check_catches_planted_mistakes():
    """net_ref.check_head_wiring (through check_wiring, as the GPU test applies it to the device's taps) passes a stand-in head that sums (box + cls)
    + angle and fails, at each of the three levels, one that drops the angle summand, one that drops the class summand and one that sums
    (box + angle) + cls -- on inputs for which that order changes at least one bit of the sum."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 64, 96, 3, generator=g).to(torch.bfloat16)
    dx_of = _branch_dx_of(g)
    kept = {}

    def d_of(head):
        def f(fs):
            kept["dx"] = dx_of(fs)
            return head.backward(kept["dx"])
        return f
    taps = NR.StandInTrunk().run(x, d_of(NR.StandInHead()))
    assert "branch_din" in taps[23] and "partial" in taps[23]
    NR.check_wiring(taps)
    NR.check_head_wiring(taps)
    for lv in range(3):
        for mistake, msg in (("drop_angle", "the sum is not"), ("drop_cls", "the partial sum is not"), ("order", "the partial sum is not")):
            with pytest.raises(AssertionError, match=rf"head level {lv}: {msg}"):
                NR.check_wiring(NR.StandInTrunk().run(x, d_of(NR.StandInHead(mistake, lv))))
            if mistake == "order":  # the inputs just used: the two orders give different bits at this level
                b, c, a = kept["dx"][lv]
                assert not NR._same(NR._add(NR._add(b, c), a), NR._add(NR._add(b, a), c))
    # a sum the trunk did not receive (the head returned something else than it recorded)
    taps = NR.StandInTrunk().run(x, d_of(NR.StandInHead()))
    taps[23]["din"] = [t.clone() for t in taps[23]["din"]]
    taps[23]["din"][1][0, 0, 0, 0] += 1.0
    with pytest.raises(AssertionError, match="head level 1"):
        NR.check_head_wiring(taps)


@pytest.mark.parametrize("scale,ch,H,W,seed", NR.MODULE_CASES, ids=lambda v: str(v))
def test_head_same_shape_layers_differ_between_levels(scale, ch, H, W, seed):
    """The layers of model.23 whose shapes are the same at all three levels hold different values at every level in the state dicts the GPU test
    uses (net_ref.make_state draws every tensor on its own), so the references built from model.23.cv3.1.1.* are not those of cv3.2.1.*: a level
    mix-up in Net.__init__ cannot pass the per-branch comparison."""
    st = NR.make_state(scale, 12, ch, seed=seed)
    n = 0
    for fam, names in NR.HEAD_SAME_SHAPE.items():
        for name in names:
            keys = [k[len(f"model.23.{fam}.0.{name}"):] for k in st if k.startswith(f"model.23.{fam}.0.{name}.")]
            assert keys
            for key in keys:
                t = [st[f"model.23.{fam}.{lv}.{name}{key}"] for lv in range(3)]
                assert t[0].shape == t[1].shape == t[2].shape, (fam, name, key)
                for i, j in ((0, 1), (0, 2), (1, 2)):
                    assert float((t[i] - t[j]).abs().max()) > 1e-2 * float(t[i].abs().max()), (fam, name, key, i, j)
                    n += 1
    assert n == 3 * (4 * 5 + 3 * 2)  # four Conv blocks of five tensors, three plain convs of two, three level pairs each
    x = torch.randn(2, 4, 4, st["model.23.cv3.1.1.0.conv.weight"].shape[0], generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    outs = []
    for lv in (1, 2):  # and the references themselves: the second class pair of levels 1 and 2 on one input
        a = x.double().permute(0, 3, 1, 2)
        for name, m in NR.head_spec(st, lv)["cls"][2:4]:
            m.reset()
            a = m(a, True)
        outs.append(a.detach())
    assert NR.DR.rel_dist(outs[0], outs[1]) > 0.5


@pytest.mark.parametrize("scale,ch,H,W,seed", NR.MODULE_CASES, ids=lambda v: str(v))
def test_head_bounds_stay_below_half(scale, ch, H, W, seed):
    """The bounds of the per-branch head test, max(FLOOR, 4 x grain), for the nine branches at the inputs they see inside the net (the rounded
    restatement chained on the CPU) under the dense seeded gradients the GPU test's second drive uses (net_ref.head_dense_grads, seed + 200), from
    the two references alone: none reaches 0.5, no quantity left out."""
    st = NR.make_state(scale, 12, ch, seed=seed)
    tiles = torch.randint(0, 256, (2, H, W, ch), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    _, outs = NR.ref_module_inputs(st, tiles)
    feats = [outs[t] for t in NR.HEAD_FROM]
    dense = NR.head_dense_grads(seed + 200, [tuple(f.shape[:3]) for f in feats], 12)
    worst = {}
    for lv, x in enumerate(feats):
        for k, kind in enumerate(NR.HEAD_KINDS):
            rounded, plain = NR.branch_refs(st, lv, kind, x, dense[k][lv])
            assert sum(n.endswith(("dW", "dgamma", "dbeta", "rmean", "rvar")) for n in rounded) == (20 if kind == "cls" else 10) + 1
            for n, b in NR.BR.bounds(rounded, plain).items():
                worst[f"{kind}.{lv}.{n}"] = b
    assert len(worst) == 3 * (2 * 14 + 24)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("  largest head bounds:", ", ".join(f"{n} {b:.3f}" for n, b in top))
    assert top[0][1] < 0.5, top
