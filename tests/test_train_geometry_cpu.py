"""The work splits of the training kernels' slab reductions, pinned: obb_dwconv3_bwd_geometry, obb_headconv_bwd_geometry and
obb_stemconv_wgrad_geometry (host-only, no context) at every YOLO11 n / s layer shape of train_shapes.py and at the edges where the split changes
branch, against tests/golden/train_geometry.json -- recorded from the build before the kernels' helpers moved into csrc/traindev.h.  The split
(rows per stripe, lane run, slabs, the fp32 chain length L that sets the GPU tests' bounds) decides the order of every fp32 addition, so a
refactor of the geometry code has to leave each number as it was.  `python tests/test_train_geometry_cpu.py` rewrites the file.  No GPU."""
import json
import os

import pytest

from conftest import GOLDEN  # (first: it puts the repository root on sys.path when this file is run as a script)
import train_shapes as TS

PATH = os.path.join(GOLDEN, "train_geometry.json")
EDGE_C = (8, 24, 256, 264)        # CW 1 (RP 256), RP 85 (no power of two), one full column group, two groups with a partial one
EDGE_SIDE = (1, 16, 17)           # 16 / 17: the depthwise stripe rule (R 2 / 4)
EDGE_COUT = (1, 4, 5, 16, 17, 64)  # the head's OT classes 4 / 16 / 64 on both sides of each threshold


def _layer_maps():
    """(B, Ho, Wo, c1, c2) of every catalogue conv of both scales, deduplicated."""
    seen = []
    for sc in ("n", "s"):
        for e in TS.conv_catalogue(sc):
            Ho, Wo = ((e.H + 1) // 2, (e.W + 1) // 2) if e.s == 2 else (e.H, e.W)
            k = (e.B, Ho, Wo, e.c1, e.c2)
            if k not in seen:
                seen.append(k)
    return seen


def dw_cases():
    """(B, H, W, C): every output map of the catalogue at its channel count, then the edges; 1 x 1024 x 1024 is the 2^20-pixel map."""
    out = [(B, H, W, c2) for B, H, W, _, c2 in _layer_maps() if c2 % 8 == 0]
    out += [(B, H, W, C) for C in EDGE_C for B in (1, 7) for H in EDGE_SIDE for W in EDGE_SIDE]
    out += [(1, 1024, 1024, C) for C in EDGE_C] + [(2, 16, 260, 256)]
    return sorted(set(out))


def head_cases():
    """(N, cin, cout): every catalogue map as the pixel count of a head output with its input channels, then the edges."""
    maps = sorted({(B * H * W, c1) for B, H, W, c1, _ in _layer_maps() if c1 % 8 == 0 and c1 <= 512})
    out = [(N, cin, cout) for N, cin in maps for cout in (1, 12, 64)]
    out += [(N, cin, cout) for N in (1, 7, 1 << 20) for cin in EDGE_C + (512,) for cout in EDGE_COUT]
    return sorted(set(out))


def stem_cases():
    """(B, H, W, cin, cout): the 416-px tile and the edges; 1 x 2048 x 2048 has 2^20 output pixels."""
    out = [(B, TS.IMGSZ, TS.IMGSZ, cin, cout) for B in (1, 2, 16) for cin in (3, 4) for cout in (16, 32)]
    out += [(B, H, W, cin, cout) for B in (1, 7) for H in EDGE_SIDE for W in EDGE_SIDE for cin in (3, 4) for cout in (8, 16, 24, 64)]
    out += [(1, 2048, 2048, cin, cout) for cin in (3, 4) for cout in (8, 64)]
    return sorted(set(out))


def _ops():
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops
    return ops


def compute():
    """-> {entry point: [[args..., out0, out1, out2, out3], ...]}"""
    ops = _ops()
    return {
        "obb_dwconv3_bwd_geometry": [list(a) + [int(v) for v in ops.dwconv3_bwd_geometry(*a)] for a in dw_cases()],
        "obb_headconv_bwd_geometry": [list(a) + [int(v) for v in ops.headconv_bwd_geometry(*a)] for a in head_cases()],
        "obb_stemconv_wgrad_geometry": [list(a) + [int(v) for v in ops.stemconv_wgrad_geometry(*a)] for a in stem_cases()],
    }


@pytest.fixture(scope="module")
def now():
    return compute()


@pytest.mark.parametrize("entry", ["obb_dwconv3_bwd_geometry", "obb_headconv_bwd_geometry", "obb_stemconv_wgrad_geometry"])
def test_geometry_is_the_recorded_one(entry, now):
    rec = json.load(open(PATH))[entry]
    assert len(rec) == len(now[entry]) and len(rec) > 100, (len(rec), len(now[entry]))
    diff = [(r, n) for r, n in zip(rec, now[entry]) if r != n]
    assert not diff, f"{len(diff)} of {len(rec)} splits moved; first (recorded, now): {diff[0]}"


def test_sweep_reaches_every_branch(now):
    """The recorded cases sit on both sides of every rule of the splits: R 2 and 4, one and several slabs, the 512-slab cap, a lane run above
    one, RP a power of two, none (21, 42) and 1, a walker with two slabs (nbx > 64) and idle walkers (nbx < 64)."""
    dw = now["obb_dwconv3_bwd_geometry"]
    assert {r[4] for r in dw} == {2, 4} and {1, 512} <= {r[6] for r in dw} and any(r[5] > r[4] for r in dw)
    for entry in ("obb_headconv_bwd_geometry", "obb_stemconv_wgrad_geometry"):
        rows = [r[-4:] for r in now[entry]]
        assert {1, 512} <= {r[2] for r in rows} and any(1 < r[2] < 64 for r in rows) and any(64 < r[2] < 512 for r in rows), entry
        assert any(r[0] > 1 for r in rows), entry
    assert {64, 21, 1} <= {r[-3] for r in now["obb_headconv_bwd_geometry"]} and {128, 42} <= {r[-3] for r in now["obb_stemconv_wgrad_geometry"]}


if __name__ == "__main__":
    with open(PATH, "w") as f:
        json.dump(compute(), f, separators=(",", ":"))
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes")
