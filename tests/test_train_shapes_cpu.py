"""The training-shape catalogue (train_shapes.py) pinned per scale: a change to the graph or to the training kernels' channel limits shows up
here as a deliberate edit."""
from collections import Counter

import pytest

import train_shapes as TS


@pytest.mark.parametrize("scale,entries,covered,wgrad", [("n", 58, 82, 55), ("s", 62, 82, 68)])
def test_catalogue_counts(scale, entries, covered, wgrad):
    layers = TS.conv_layers(scale)
    assert len(layers) == 96
    assert len(TS.conv_catalogue(scale)) == entries
    cls = Counter(TS.conv_class(k, s, g, c1, c2) for _, k, s, g, c1, c2, _, _ in layers)
    assert cls[TS.COVERED] + cls[TS.WGRAD] == covered
    assert cls[TS.WGRAD] == wgrad
    # no training kernel yet: 7 depthwise convs, the cin = 3 stem, three 12-channel class outputs, three 1-channel angle outputs
    gaps = [(g, c1, c2) for _, k, s, g, c1, c2, _, _ in layers if TS.conv_class(k, s, g, c1, c2) == TS.GAP]
    assert len(gaps) == 96 - covered == 14
    assert sum(g > 1 for g, _, _ in gaps) == 7
    assert sum(c1 == 3 for _, c1, _ in gaps) == 1
    assert sum(g == 1 and c2 == 12 for g, _, c2 in gaps) == 3 and sum(g == 1 and c2 == 1 for g, _, c2 in gaps) == 3


def test_catalogue_shapes():
    """Stride-2 input maps are twice the output map; every entry is in exactly one class; the BN layers exclude the 9 head outputs."""
    for scale in ("n", "s"):
        for name, k, s, g, c1, c2, H, W in TS.conv_layers(scale):
            assert k in (1, 3) and s in (1, 2) and H == W and TS.IMGSZ % H == 0
            assert TS.conv_class(k, s, g, c1, c2) in (TS.COVERED, TS.WGRAD, TS.GAP)
        assert sum(TS.is_bn(n) for n, *_ in TS.conv_layers(scale)) == 96 - 9
        ids = [e.id for e in TS.conv_catalogue(scale)]
        assert len(set(ids)) == len(ids) and all(i.startswith(scale + ":model.") for i in ids)
    assert {e.C for e in TS.EDGE_BNS} >= {8, 24, 48, 264, 392}
    assert any(e.B * e.H * e.W == 2 for e in TS.EDGE_BNS)
    assert any(e.k == 1 and (e.B * e.H * e.W) % 128 for e in TS.EDGE_CONVS)

