"""Layer-shape catalogue of the training kernels: every conv / BatchNorm shape of YOLO11 n and s at 416 x 416, derived from the oracle graph
(`Yolo11OBB(scale).convs` + `_trace_sizes`), plus off-catalogue edge shapes where the kernels change branch (map sides, tile forms, channel
groups, pixel counts).  Used by test_train_shapes_cpu.py (the class counts) and test_gpu_train_shapes.py (the kernels at each shape)."""
from collections import namedtuple

from oracle.yolo11_obb import Yolo11OBB

IMGSZ = 416
# one dense conv: kernel k, stride s, groups g, c1 -> c2, INPUT map H x W (a stride-2 conv's output is (H + 1) // 2), batch B of the tests
ConvShape = namedtuple("ConvShape", "id k s g c1 c2 H W B")
BnShape = namedtuple("BnShape", "id C B H W")

COVERED, WGRAD, GAP = "covered", "wgrad", "gap"


def _batch(H, W):
    return 1 if H * W >= 208 * 208 else 2  # small batches keep the module to a few minutes; 1 for the largest maps


def conv_class(k, s, g, c1, c2):
    """GAP: no training kernel yet (depthwise, the cin = 3 stem, the 12- and 1-channel head outputs); WGRAD: covered and both channel counts
    multiples of 64 (one wgrad workgroup = a 64 x 64 block of dW); COVERED: dense with c1, c2 multiples of 8 (fwd / dgrad / BN only)."""
    if g != 1 or c1 % 8 or c2 % 8:
        return GAP
    return WGRAD if c1 % 64 == 0 and c2 % 64 == 0 else COVERED


def is_bn(name):
    """Every conv is Conv2d -> BatchNorm2d (-> SiLU) except the plain nn.Conv2d outputs of the head (model.23.cv{2,3,4}.i.2)."""
    p = name.split(".")
    return not (p[1] == "23" and len(p) == 5 and p[4] == "2")


def conv_layers(scale, h=IMGSZ, w=IMGSZ):
    """-> [(name, k, s, g, c1, c2, H, W)] of all convs of the model, H x W the input map."""
    m = Yolo11OBB(scale)
    sizes = m._trace_sizes(h, w)
    out = []
    for name, r in m.convs.items():
        ho, wo = sizes[name]
        H, W = (2 * ho, 2 * wo) if r.s == 2 else (ho, wo)
        out.append((name, r.k, r.s, r.g, r.c1, r.c2, H, W))
    return out


def conv_catalogue(scale):
    """Deduplicated on (k, s, g, c1, c2, H, W); the id names the first layer of each shape, e.g. "n:model.2.m.0.cv1"."""
    seen, cat = set(), []
    for name, k, s, g, c1, c2, H, W in conv_layers(scale):
        if (k, s, g, c1, c2, H, W) not in seen:
            seen.add((k, s, g, c1, c2, H, W))
            cat.append(ConvShape(f"{scale}:{name}", k, s, g, c1, c2, H, W, _batch(H, W)))
    return cat


def bn_catalogue(scale):
    """BatchNorm layers deduplicated on (C, output map)."""
    seen, cat = set(), []
    for name, k, s, g, c1, c2, H, W in conv_layers(scale):
        if not is_bn(name):
            continue
        Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if s == 2 else (H, W)
        if (c2, Ho, Wo) not in seen:
            seen.add((c2, Ho, Wo))
            cat.append(BnShape(f"{scale}:{name}", c2, _batch(H, W), Ho, Wo))
    return cat


def trained_convs():
    """Catalogue entries of both scales that have training kernels, deduplicated across the scales."""
    seen, out = set(), []
    for sc in ("n", "s"):
        for e in conv_catalogue(sc):
            key = (e.k, e.s, e.c1, e.c2, e.H, e.W)
            if conv_class(e.k, e.s, e.g, e.c1, e.c2) != GAP and key not in seen:
                seen.add(key)
                out.append(e)
    return out


def trained_bns():
    seen, out = set(), []
    for sc in ("n", "s"):
        for e in bn_catalogue(sc):
            if (e.C, e.H, e.W) not in seen:
                seen.add((e.C, e.H, e.W))
                out.append(e)
    return out


# ---- off-catalogue edge shapes: (id, k, s, g, c1, c2, H, W, B)
EDGE_CONVS = [ConvShape(*a) for a in [
    # non-square maps of the 416 x 288 tile (52 x 36, 26 x 18, 13 x 9): a swapped H / W index fails here
    ("edge:3x3 64-64 52x36", 3, 1, 1, 64, 64, 52, 36, 2),
    ("edge:3x3 32-32 26x18", 3, 1, 1, 32, 32, 26, 18, 2),
    ("edge:3x3 128-64 13x9", 3, 1, 1, 128, 64, 13, 9, 2),
    ("edge:1x1 64-128 26x18", 1, 1, 1, 64, 128, 26, 18, 2),
    ("edge:s2 64-128 52x36", 3, 2, 1, 64, 128, 52, 36, 2),
    ("edge:s2 128-128 26x18", 3, 2, 1, 128, 128, 26, 18, 2),
    # the 128-px levels; 8 x 8 / 4 x 4 below 16 and not multiples of 13: the 8 x 8 tile and the register-direct store path
    ("edge:3x3 64-64 16x16", 3, 1, 1, 64, 64, 16, 16, 2),
    ("edge:3x3 128-128 8x8", 3, 1, 1, 128, 128, 8, 8, 2),
    ("edge:3x3 64-32 8x8", 3, 1, 1, 64, 32, 8, 8, 2),
    ("edge:3x3 256-256 4x4", 3, 1, 1, 256, 256, 4, 4, 2),
    ("edge:3x3 64-16 4x4", 3, 1, 1, 64, 16, 4, 4, 3),
    # odd maps at stride 2
    ("edge:s2 64-64 27x13", 3, 2, 1, 64, 64, 27, 13, 2),
    ("edge:s2 128-128 7x5", 3, 2, 1, 128, 128, 7, 5, 2),
    # tiny maps
    ("edge:3x3 64-64 1x1", 3, 1, 1, 64, 64, 1, 1, 2),
    ("edge:3x3 64-64 2x2", 3, 1, 1, 64, 64, 2, 2, 2),
    ("edge:3x3 64-64 2x1", 3, 1, 1, 64, 64, 2, 1, 2),
    ("edge:s2 64-64 2x1", 3, 2, 1, 64, 64, 2, 1, 2),
    ("edge:s2 64-64 1x1", 3, 2, 1, 64, 64, 1, 1, 3),
    # batch 1
    ("edge:3x3 64-64 26x26 B1", 3, 1, 1, 64, 64, 26, 26, 1),
    ("edge:s2 64-64 26x26 B1", 3, 2, 1, 64, 64, 26, 26, 1),
    # 1x1 with B*H*W not a multiple of 128 (the one long pixel row of the 1x1 path ends inside a tile)
    ("edge:1x1 64-64 13x9", 1, 1, 1, 64, 64, 13, 9, 2),
    ("edge:1x1 32-16 7x5 B1", 1, 1, 1, 32, 16, 7, 5, 1),
    ("edge:1x1 256-64 5x3", 1, 1, 1, 256, 64, 5, 3, 3),
    ("edge:1x1 64-8 1x1", 1, 1, 1, 64, 8, 1, 1, 1),
    # 3x3 on 13-multiple maps with cin 32 / 64 and cout <= 32: plan_conv's single-stage weights-resident (WRES) form, non-square included
    ("edge:wres 32-16 26x26", 3, 1, 1, 32, 16, 26, 26, 2),
    ("edge:wres 32-32 13x13", 3, 1, 1, 32, 32, 13, 13, 2),
    ("edge:wres 64-16 52x52", 3, 1, 1, 64, 16, 52, 52, 2),
    ("edge:wres 64-32 39x13", 3, 1, 1, 64, 32, 39, 13, 2),
    ("edge:wres 64-32 13x26", 3, 1, 1, 64, 32, 13, 26, 2),
]]

# BatchNorm channel counts off the catalogue: CW = C / 8 not a power of two (24, 48: idle threads in the 256-thread workgroup), more than one
# 256-channel group with a partial last one (264, 392); (C, B, H, W)
EDGE_BNS = [BnShape(f"edge:bn C{C} {B}x{H}x{W}", C, B, H, W) for C, B, H, W in
            [(8, 2, 52, 52), (24, 2, 26, 26), (48, 2, 13, 9), (264, 2, 13, 13), (392, 2, 26, 18), (64, 1, 2, 1)]]
