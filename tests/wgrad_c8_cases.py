"""Shapes of the weight-gradient kernel at multiples of 8 (csrc/convgrad.hip, k_conv_wgrad / obb_conv_wgrad_c8_bf16), shared by
test_train_wgrad_c8_cpu.py (the lists against the catalogue) and test_gpu_train_wgrad_c8.py (the kernel at each of them).

NARROW_SHAPES: the dense conv shapes of YOLO11 n and s at 416 x 416 that have forward / dgrad kernels but whose channel counts are not both
multiples of 64 -- (k, s, c1, c2, H, W), H x W the input map, deduplicated across the two scales, in catalogue order.  NARROW_PAIRS: their
distinct (k, s, c1, c2).  The GPU tests run the pairs at small maps; the full maps differ only in the number of tiles a walker takes."""
from collections import namedtuple

NARROW_SHAPES = [
    (3, 2, 16, 32, 208, 208), (1, 1, 32, 32, 104, 104), (1, 1, 48, 64, 104, 104), (3, 1, 16, 8, 104, 104), (3, 1, 8, 16, 104, 104),
    (1, 1, 96, 128, 52, 52), (3, 1, 32, 16, 52, 52), (3, 1, 16, 32, 52, 52), (1, 1, 64, 32, 26, 26), (3, 1, 32, 32, 26, 26),
    (3, 1, 64, 32, 26, 26), (3, 1, 32, 64, 26, 26), (1, 1, 96, 64, 52, 52), (3, 1, 64, 16, 52, 52), (3, 1, 16, 16, 52, 52),
    (3, 1, 128, 16, 26, 26), (3, 1, 16, 16, 26, 26), (3, 1, 256, 16, 13, 13), (3, 1, 16, 16, 13, 13),
    (3, 2, 32, 64, 208, 208), (1, 1, 96, 128, 104, 104), (3, 1, 32, 16, 104, 104), (3, 1, 16, 32, 104, 104), (3, 1, 64, 32, 52, 52),
    (3, 1, 32, 64, 52, 52), (3, 1, 128, 32, 52, 52), (3, 1, 32, 32, 52, 52), (3, 1, 256, 32, 26, 26), (3, 1, 512, 32, 13, 13),
    (3, 1, 32, 32, 13, 13),
]
N_NARROW_SHAPES = 30


def _distinct(seq):
    seen, out = set(), []
    for t in seq:
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


NARROW_PAIRS = _distinct(t[:4] for t in NARROW_SHAPES)
N_NARROW_PAIRS = 21

# one GPU case: kernel k, stride s, c1 -> c2, batch B, INPUT map H x W
Case = namedtuple("Case", "group k s c1 c2 B H W")


def case_id(c):
    return f"{c.group}:{'s2' if c.s == 2 else f'{c.k}x{c.k}'} {c.c1}-{c.c2} {c.B}x{c.H}x{c.W}"


def _cross(group, shapes, maps):
    return [Case(group, k, s, c1, c2, B, H, W) for (k, s, c1, c2) in shapes for (B, H, W) in maps]


S2_NARROW = [(3, 2, 16, 32), (3, 2, 32, 64)]
GPU_CASES = (
    # every narrow channel pair of the catalogue on a non-square map with Wo % 4 != 0
    _cross("pair", NARROW_PAIRS, [(2, 13, 9)])
    # one fragment / half a fragment per side; 1 x 26 x 18: several tiles, more than one row per tile
    + _cross("frag", [(3, 1, 16, 8), (3, 1, 8, 16), (3, 1, 8, 8), (1, 1, 8, 8)], [(2, 7, 5), (1, 1, 1), (2, 2, 1), (1, 26, 18)])
    # a partial last block next to a full one, on either side and on both
    + _cross("partial", [(1, 1, 96, 128), (1, 1, 48, 64), (1, 1, 72, 136), (3, 1, 136, 72)], [(2, 13, 9), (3, 5, 3)])
    # wide rows: the LDS tile at the live width (model.1's 208-pixel row at stride 2, the 104-pixel rows of model.2's Bottleneck)
    + _cross("wide", S2_NARROW, [(1, 4, 208)]) + _cross("wide", [(3, 1, 16, 8), (3, 1, 8, 16)], [(1, 3, 104)])
    # stride 2 on odd and tiny maps
    + _cross("s2odd", S2_NARROW, [(2, 27, 13), (2, 7, 5), (2, 2, 1), (3, 1, 1)])
    # multiples of 64 through the same entry
    + _cross("c64", [(3, 1, 64, 64), (1, 1, 128, 64), (3, 2, 64, 128)], [(2, 13, 9)])
    # a single row beyond 64 KiB of LDS (3 x 209 X pixels + 104 dY pixels of 64 channels = 91.4 KiB): the raised cap
    + _cross("lds>64K", [(3, 2, 64, 64)], [(1, 2, 208)])
)

# inputs with a known answer, one per (k, s) at 16 -> 8 (a narrow block) and at 64 -> 64 (the kernel instance with compile-time widths)
EXACT_CASES = _cross("exact", [(1, 1, 16, 8), (3, 1, 16, 8), (3, 2, 16, 8), (3, 1, 64, 64), (1, 1, 64, 64), (3, 2, 64, 64)], [(2, 13, 9)])

# multiples of 64, where obb_conv_wgrad_bf16 / obb_conv_wgrad_s2_bf16 and obb_conv_wgrad_c8_bf16 must give the same bits; 1 x 26 x 18 at
# 128 -> 128: several tiles per walker, more than one row per tile, four blocks
ENTRY_EQUALITY_CASES = (_cross("entries", [(3, 1, 64, 64), (1, 1, 128, 64), (3, 2, 64, 128)], [(2, 13, 9)])
                        + _cross("entries", [(3, 1, 128, 128)], [(1, 26, 18)]))

# train.ConvBN end to end: (k, s, c1, c2, B, H, W)
CONVBN_CASES = [(3, 1, 16, 8, 2, 13, 9), (1, 1, 48, 64, 2, 13, 9), (3, 2, 16, 32, 2, 8, 6)]
