"""The one structure walk of train.py (`children()` -> `named_blocks()` -> `fold()`, `Net.pack_layers`, `FoldPlan`) without a GPU: no kernel
runs, the constructors only register CPU tensors.

  * walk invariants, for every kind of test_train_layout_cpu.KINDS that has children and for whole nets: unique names, fold() keyed exactly by
    named_blocks(), name order = registration order (the own-groups DetectHead is the one exception, and its order is stated here), and every
    name = the parent's child name + "." + the child's own name, down to the leaves;
  * `FoldPlan(net)` on a CPU-built net against tests/golden/fold_plan.json: the header and record table bytes, the kernel records and the
    names as the commit BEFORE the walk was unified wrote them (`python tests/test_train_walk_cpu.py` writes the fixture from the code it is run
    in, through attributes that exist on both sides of that change);
  * `Net.pack_layers(H, W)` against net_ref's own table of input strides, looked up by each layer's name."""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fold_plan.json")
NETS = [("n", 3), ("n", 4), ("s", 3), ("s", 4)]


def _net(scale, ch, nc=12, seed=5):
    import net_ref as NR
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import train
    return train.Net.from_state(NR.make_state(scale, nc, ch, seed=seed), scale, nc, ch)


# ---------------------------------------------------------------------------------------------- walk invariants
def _is_composite(m):
    return hasattr(m, "children")


def _check_names_compose(mod):
    """named_blocks() of `mod` is, child by child, the child itself under its own name (a leaf) or the child's named_blocks() behind
    "<child name>." (a composite): no composite invents, drops or reorders names.  Recursive."""
    want = []
    for name, c in mod.children():
        assert name and not name.startswith(".") and not name.endswith("."), name
        if _is_composite(c):
            _check_names_compose(c)
            sub = c.named_blocks()
            assert sub, name
            want += [(f"{name}.{n}", b) for n, b in sub]
        else:
            assert not hasattr(c, "named_blocks"), name  # a leaf lists nothing
            want.append((name, c))
    got = mod.named_blocks()
    assert [n for n, _ in got] == [n for n, _ in want]
    assert all(a is b for (_, a), (_, b) in zip(got, want))


def _check_walk(mod, registration=None):
    blocks = mod.named_blocks()
    names = [n for n, _ in blocks]
    assert names and len(set(names)) == len(names)
    assert len({id(b) for _, b in blocks}) == len(blocks)
    assert list(mod.fold()) == names
    iw = [b._iw for _, b in blocks]
    if registration is None:
        assert all(a < b for a, b in zip(iw, iw[1:])), "named_blocks() is not in registration order"
    else:
        assert [n for _, n in sorted(zip(iw, names))] == registration
    _check_names_compose(mod)


def _composite_kinds():
    import test_train_layout_cpu as TL
    import oriented_object_detection_amd.train as TR
    out = []
    for kind in TL.KINDS:
        mod, _ = TL.KINDS[kind](TR, TL._Draw(kind))
        if hasattr(mod, "named_blocks"):
            out.append((kind, mod))
    return out


def test_walk_invariants_of_every_composite_kind():
    kinds = _composite_kinds()
    # every kind that is no single layer has children
    assert sorted(k for k, _ in kinds) == sorted(["class_pair", "attention", "psablock", "c2psa", "sppf", "bottleneck", "c3k", "c3k2_n2", "c3k2_n2_c3k",
                                                  "angle_branch", "box_step", "class_step", "detect_head"])
    for kind, mod in kinds:
        registration = None
        if kind == "detect_head":  # on groups of its own the head registers per level box, class, angle; its names list in checkpoint order
            names = [n for n, _ in mod.named_blocks()]
            registration = [n for lv in range(3) for cv in ("cv2", "cv3", "cv4") for n in names if n.startswith(f"{cv}.{lv}.")]
            assert sorted(registration) == sorted(names) and registration != names
            assert [n.split(".")[0] for n in names] == ["cv2"] * 9 + ["cv3"] * 15 + ["cv4"] * 9
        _check_walk(mod, registration)


@pytest.mark.parametrize("scale,ch", NETS, ids=lambda v: str(v))
def test_walk_invariants_of_the_net(scale, ch):
    net = _net(scale, ch)
    _check_walk(net)
    _check_walk(net.trunk)
    top = [n for n, _ in net.children()]
    assert top == [n for n, _ in net.trunk.children()] + ["model.23." + n for n, _ in net.head.children()]
    assert [n for n, _ in net.head.children()] == [f"{cv}.{i}" for cv in ("cv2", "cv3", "cv4") for i in range(3)]
    # the qkv blocks fold to checkpoint order by themselves: the composites add nothing to a leaf's fold()
    fold = net.fold()
    for name, b in net.named_blocks():
        w, bias = b.fold()
        assert torch.equal(fold[name][0], w) and torch.equal(fold[name][1], bias), name


# ---------------------------------------------------------------------------------------------- FoldPlan against the recorded one
def fold_plan_of(scale):
    """-> {"head_sha256", "records_sha256", "names"} of FoldPlan(net) for the net of `scale` at nc = 12, ch = 3 (CPU-built)"""
    from oriented_object_detection_amd import train
    plan = train.FoldPlan(_net(scale, 3))
    return {"head_sha256": hashlib.sha256(bytes(plan.blob[:plan.data_off])).hexdigest(),
            "records_sha256": hashlib.sha256(repr(plan.records).encode()).hexdigest(),
            "names": list(plan.names)}


@pytest.mark.parametrize("scale", ["n", "s"])
def test_fold_plan_is_the_recorded_one(scale):
    with open(FIXTURE) as f:
        want = json.load(f)[scale]
    got = fold_plan_of(scale)
    assert got["names"] == want["names"]
    assert got["records_sha256"] == want["records_sha256"], "the fold kernel's records (kind, offsets, c2, per) changed"
    assert got["head_sha256"] == want["head_sha256"], "the blob's header or record table (names, c1, c2, k, s, g, act, offsets) changed"


def test_fold_plan_rejects_another_row_order():
    """The fold kernel knows one permutation, argsort(qkv_device_order(c2 // 128)): a leaf whose row order is set to anything else is refused."""
    from oriented_object_detection_amd import train
    net = _net("n", 3)
    qkv = net.trunk.m[10].m[0].attn.qkv
    assert torch.equal(qkv.order, torch.argsort(train.qkv_device_order(qkv.c2 // 128)))
    qkv.order = qkv.order.flip(0)
    with pytest.raises(ValueError):
        train.FoldPlan(net)


# ---------------------------------------------------------------------------------------------- pack maps
@pytest.mark.parametrize("scale,ch", NETS, ids=lambda v: str(v))
def test_pack_layers_against_net_refs_strides(scale, ch):
    import net_ref as NR
    net = _net(scale, ch)
    blocks = net.named_blocks()
    name_of = {id(b): n for n, b in blocks}
    packed = [b for _, b in blocks if hasattr(b, "_packed")]
    assert packed
    for H, W in ((32, 32), (64, 96), (416, 416)):
        got = net.pack_layers(H, W)
        assert [id(b) for b, _ in got] == [id(b) for b in packed]  # exactly the leaves with `_packed`, in the walk's order
        for b, hw in got:
            parts = name_of[id(b)].split(".")
            lv = (8, 16, 32)[int(parts[3])] if parts[1] == "23" else NR.IN_LEVEL[int(parts[1])]
            assert hw == (H // lv, W // lv), (name_of[id(b)], hw)
        # net_ref's own list of the dense layers names the same layers with the same maps
        assert {(name_of[id(b)], *hw) for b, hw in got} == {(n, h, w) for n, _, _, _, _, h, w in NR.dense_layers(scale, 12, ch, H, W)}


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    with open(FIXTURE, "w") as f:
        json.dump({s: fold_plan_of(s) for s in ("n", "s")}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {FIXTURE}")
