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
