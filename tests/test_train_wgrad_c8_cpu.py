"""CPU checks of the multiple-of-8 weight gradient (obb_conv_wgrad_c8_bf16, ops.conv_wgrad_c8_bf16, train.wgrad_route): the entry point is
exported, declared and bound; every dense conv of YOLO11 n / s that has forward and dgrad kernels gets a weight-gradient route; the test
helper's shape lists are the catalogue's."""
import os
import re
from collections import Counter

import pytest

import train_shapes as TS
import wgrad_c8_cases as WC
from conftest import ROOT

NAME = "obb_conv_wgrad_c8_bf16"


def test_entry_point_is_exported_declared_and_bound():
    import __graft_entry__ as g
    g._load_build_module().build()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "obbhip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{NAME} is not declared in include/obbhip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "x", "dy", "B", "H", "W", "cin", "cout", "ks", "stride", "dw", "s"]
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME]) == len(args)
    assert hasattr(_lib.lib(), NAME), f"{NAME} is not exported by the built library"
    assert callable(ops.conv_wgrad_c8_bf16)
    # the two older entry points keep their arguments
    assert len(_lib.SIGNATURES["obb_conv_wgrad_bf16"]) == 11 and len(_lib.SIGNATURES["obb_conv_wgrad_s2_bf16"]) == 10


@pytest.mark.parametrize("scale,c8", [("n", 27), ("s", 14)])
def test_every_covered_layer_has_a_wgrad_route(scale, c8):
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd.train import wgrad_route
    routes = Counter()
    for name, k, s, g, c1, c2, H, W in TS.conv_layers(scale):
        cls = TS.conv_class(k, s, g, c1, c2)
        if cls == TS.GAP:
            continue
        r = wgrad_route(c1, c2)
        assert r == ("c64" if cls == TS.WGRAD else "c8"), (name, c1, c2, r)
        routes[r] += 1
    assert routes["c64"] + routes["c8"] == 82
    assert routes["c8"] == c8


def test_wgrad_route_refuses_what_has_no_kernel():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd.train import wgrad_route
    assert wgrad_route(64, 64) == "c64" and wgrad_route(128, 512) == "c64"
    assert wgrad_route(64, 8) == "c8" and wgrad_route(8, 64) == "c8" and wgrad_route(72, 136) == "c8"
    for c1, c2 in ((3, 16), (64, 12), (64, 1), (0, 64), (64, 0), (4, 8)):
        with pytest.raises(ValueError, match="multiples of 8"):
            wgrad_route(c1, c2)


def test_narrow_shape_lists_are_the_catalogues():
    assert len(WC.NARROW_SHAPES) == WC.N_NARROW_SHAPES == 30
    assert len(WC.NARROW_PAIRS) == WC.N_NARROW_PAIRS == 21
    cat = [(e.k, e.s, e.c1, e.c2, e.H, e.W) for e in TS.trained_convs() if TS.conv_class(e.k, e.s, e.g, e.c1, e.c2) == TS.COVERED]
    assert cat == WC.NARROW_SHAPES
    pairs = {(3, 2): [(16, 32), (32, 64)],
             (1, 1): [(32, 32), (48, 64), (96, 128), (96, 64), (64, 32)],
             (3, 1): [(16, 8), (8, 16), (32, 16), (16, 32), (32, 32), (64, 32), (32, 64), (64, 16), (16, 16), (128, 16), (256, 16), (128, 32), (256, 32),
                      (512, 32)]}
    assert set(WC.NARROW_PAIRS) == {(k, s, c1, c2) for (k, s), cc in pairs.items() for c1, c2 in cc}


def test_gpu_case_lists():
    """Every group of the kernel's test plan is there, ids are unique, and the groups hold what their names say."""
    ids = [WC.case_id(c) for c in WC.GPU_CASES]
    assert len(set(ids)) == len(ids)
    n = Counter(c.group for c in WC.GPU_CASES)
    assert n == {"pair": 21, "frag": 16, "partial": 8, "wide": 4, "s2odd": 8, "c64": 3, "lds>64K": 1}
    for c in WC.GPU_CASES:
        assert c.c1 % 8 == 0 and c.c2 % 8 == 0 and (c.k, c.s) in ((1, 1), (3, 1), (3, 2))
        if c.group == "partial":
            assert (c.c1 % 64 or c.c2 % 64) and max(c.c1, c.c2) >= 64
        if c.group == "c64":
            assert c.c1 % 64 == 0 and c.c2 % 64 == 0
    assert any(((c.W + c.s - 1) // c.s) % 4 for c in WC.GPU_CASES if c.group == "pair")
    for cc in ((16, 8), (64, 64)):  # a narrow block and the full x full instance, each at every (k, s)
        assert sorted((c.k, c.s) for c in WC.EXACT_CASES if (c.c1, c.c2) == cc) == [(1, 1), (3, 1), (3, 2)]
    assert len(WC.EXACT_CASES) == 6
    assert [(c.k, c.s, c.c1, c.c2, c.B, c.H, c.W) for c in WC.ENTRY_EQUALITY_CASES] == [
        (3, 1, 64, 64, 2, 13, 9), (1, 1, 128, 64, 2, 13, 9), (3, 2, 64, 128, 2, 13, 9), (3, 1, 128, 128, 1, 26, 18)]
