"""The parameter layout of every module kind of train.py against a recorded one (tests/golden/train_layout.json): the order, group and shape of every
`groups.add`, the bytes of the three flat parameter buffers after `build()`, and the names `named_blocks()` lists.  Optimiser state and the buckets
of `allreduce_gradients` are laid out by exactly this, so a module whose blocks register in another order trains, but not from a saved state and
not next to a rank that runs the older code.  No kernel runs: the constructors take CPU tensors.

The values are integers / 4096 drawn by `torch.randint` from a generator seeded per kind: exact in fp32 and the same on every machine, and distinct
per element, so two blocks of one shape that change places change the hash.  The qkv block of Attention is held in device channel order: its
permutation is part of what the hashes pin.

`python tests/test_train_layout_cpu.py` writes the fixture from the code it is run in."""
import hashlib
import json
import os
import sys
import zlib

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "train_layout.json")


class _Draw:
    """The tensors of one kind, drawn in order from one seeded generator."""

    def __init__(self, kind):
        self.g = torch.Generator().manual_seed(zlib.crc32(kind.encode()))

    def t(self, *shape, lo=-4096, hi=4096, add=0.0):
        return torch.randint(lo, hi, shape, generator=self.g).float() / 4096 + add

    def bn(self, c2, c1, k, n=5):
        """(w, gamma, beta, running_mean, running_var)[:n] of a dense Conv block c1 -> c2"""
        return (self.t(c2, c1, k, k), self.t(c2, lo=0, add=0.5), self.t(c2), self.t(c2), self.t(c2, lo=0, add=0.5))[:n]

    def dw(self, c, n=5):
        return (self.t(c, 1, 3, 3), self.t(c, lo=0, add=0.5), self.t(c), self.t(c), self.t(c, lo=0, add=0.5))[:n]

    def out(self, cout, c):
        """(w3, b3) of a branch's 1x1 + bias output"""
        return self.t(cout, c, 1, 1), self.t(cout)

    def psa(self):
        """(qkv, proj, pe, ffn0, ffn1) of a PSABlock with one head (64 channels)"""
        return self.bn(128, 64, 1), self.bn(64, 64, 1), self.dw(64), self.bn(128, 64, 1), self.bn(64, 128, 1)

    def c3k(self, c):
        return self.bn(c // 2, c, 1), self.bn(c // 2, c, 1), self.bn(c, c, 1), [(self.bn(c // 2, c // 2, 3), self.bn(c // 2, c // 2, 3))]

    def box(self, c):
        return [self.bn(c, c, 3, 3), self.bn(c, c, 3, 3)], *self.out(64, c)

    def cls(self, c, nc):
        return [(self.dw(c), self.bn(c, c, 1)) for _ in range(2)], *self.out(nc, c)

    def angle(self, c):
        return [self.bn(8, c, 3, 3), self.bn(8, 8, 3, 3)], *self.out(1, 8)


def _on_groups(make):
    """a module that registers in the caller's ParamGroups"""
    def build(TR, d):
        groups = TR.ParamGroups()
        mod = make(TR, d, groups)
        groups.build()
        return mod, groups
    return build


def _own_groups(make):
    """a *Step class or DetectHead: it owns (and has built) its groups"""
    def build(TR, d):
        mod = make(TR, d)
        return mod, mod.groups
    return build


# the smallest shapes each constructor accepts (channel counts in multiples of 8, one head of 64 channels)
KINDS = {
    "convbn_k1_s1": _on_groups(lambda TR, d, g: TR.ConvBN(g, *(p := d.bn(16, 8, 1))[:3], 1, *p[3:])),
    "convbn_k3_s1": _on_groups(lambda TR, d, g: TR.ConvBN(g, *d.bn(16, 8, 3)[:3])),
    "convbn_k3_s2": _on_groups(lambda TR, d, g: TR.ConvBN(g, *d.bn(16, 8, 3)[:3], 2)),
    "convbn_k1_noact": _on_groups(lambda TR, d, g: TR.ConvBN(g, d.bn(16, 8, 1)[0], act=False)),
    "dwconvbn_act": _on_groups(lambda TR, d, g: TR.DWConvBN(g, *(p := d.dw(8))[:3], True, *p[3:])),
    "dwconvbn_noact": _on_groups(lambda TR, d, g: TR.DWConvBN(g, *d.dw(8)[:3], False)),
    "stem_cin3": _on_groups(lambda TR, d, g: TR.StemConvBN(g, *d.bn(8, 3, 3))),
    "stem_cin4": _on_groups(lambda TR, d, g: TR.StemConvBN(g, *d.bn(8, 4, 3)[:3])),
    "head_out": _on_groups(lambda TR, d, g: TR.HeadOut(g, *d.out(3, 8))),
    "class_pair": _on_groups(lambda TR, d, g: TR.ClassBranchPair(g, d.dw(8), d.bn(16, 8, 1))),
    "attention": _on_groups(lambda TR, d, g: TR.Attention(g, *d.psa()[:3], 1)),
    "psablock": _on_groups(lambda TR, d, g: TR.PSABlock(g, *d.psa(), 1)),
    "c2psa": _on_groups(lambda TR, d, g: TR.C2PSA(g, d.bn(128, 128, 1), d.bn(128, 128, 1), [d.psa(), d.psa()], 1)),
    "sppf": _on_groups(lambda TR, d, g: TR.SPPF(g, d.bn(8, 16, 1), d.bn(16, 32, 1))),
    "bottleneck": _on_groups(lambda TR, d, g: TR.Bottleneck(g, d.bn(8, 16, 3), d.bn(16, 8, 3))),
    "c3k": _on_groups(lambda TR, d, g: TR.C3k(g, *d.c3k(16))),
    "c3k2_n2": _on_groups(lambda TR, d, g: TR.C3k2(g, d.bn(32, 16, 1), d.bn(16, 64, 1), [(d.bn(8, 16, 3), d.bn(16, 8, 3)) for _ in range(2)])),
    "c3k2_n2_c3k": _on_groups(lambda TR, d, g: TR.C3k2(g, d.bn(32, 16, 1), d.bn(16, 64, 1), [d.c3k(16) for _ in range(2)], c3k=True)),
    "angle_branch": _on_groups(lambda TR, d, g: TR.DetectAngleBranch(g, *d.angle(16))),
    "box_step": _own_groups(lambda TR, d: TR.DetectBoxBranchStep(*d.box(16))),
    "class_step": _own_groups(lambda TR, d: TR.DetectClassBranchStep(*d.cls(16, 3))),
    "detect_head": _own_groups(lambda TR, d: TR.DetectHead([{"box": d.box(c), "cls": d.cls(c, 3), "angle": d.angle(c)} for c in (16, 24, 32)], 3)),
}


def layout_of(kind):
    """-> {"items": [[group, shape]], "param_sha256": [three hex digests], "named_blocks": [names], or None for a single layer: a leaf lists nothing}"""
    import oriented_object_detection_amd.train as TR
    mod, groups = KINDS[kind](TR, _Draw(kind))
    named = [n for n, _ in mod.named_blocks()] if hasattr(mod, "named_blocks") else None
    return {"items": [[g, list(t.shape)] for g, t in groups.items],
            "param_sha256": [hashlib.sha256(o.param.contiguous().numpy().tobytes()).hexdigest() for o in groups.opts],
            "named_blocks": named}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_kind_is_recorded(recorded):
    assert sorted(recorded) == sorted(KINDS)


@pytest.mark.parametrize("kind", list(KINDS))
def test_layout_is_the_recorded_one(kind, recorded):
    got, want = layout_of(kind), recorded[kind]
    assert got["items"] == want["items"], f"{kind}: the order, group or shape of the registered parameters changed"
    assert got["named_blocks"] == want["named_blocks"], f"{kind}: named_blocks() lists other names"
    assert got["param_sha256"] == want["param_sha256"], f"{kind}: the flat parameter buffers hold other bytes (blocks of one shape exchanged?)"


def test_the_drawn_values_tell_blocks_apart():
    """Two blocks of one shape must not draw the same tensor, or their exchange would leave the hashes as they are."""
    d = _Draw("c3k2_n2")
    a, b = d.bn(8, 16, 3), d.bn(8, 16, 3)
    assert all(not torch.equal(x, y) for x, y in zip(a, b))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    with open(FIXTURE, "w") as f:
        json.dump({k: layout_of(k) for k in KINDS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {FIXTURE}")
