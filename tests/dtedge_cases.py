"""Inputs of the 4-channel input builder's stage tests, and a classifier of what each input asks of the device's radix select.

Every image is built from a recipe (kind, h, w, seed); no array is stored.  `classify` works from the CPU oracle's values alone: for the
q-th percentile of n values, numpy interpolates between the order statistics `rank = floor((n - 1) q / 100)` and `rank + 1`; the device's
k_dt_select finds the second one -- the "successor" -- in one of four places, named here by how many leading bits the two float bit
patterns share:
    tie    the same key (the rank-th key occurs again at rank + 1)
    low    another key under the same 22-bit prefix        (the next non-empty bin of the last radix pass)
    mid    the same top digit (bits 31..20), higher middle digit                    (s_above[q][0])
    top    a higher top digit                                                       (s_above[q][1])
"""
import functools
import math

import numpy as np

from oracle import dtedge as od

SOURCES = ("tie", "low", "mid", "top")


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def blobs(h, w, seed):
    """a few dark rectangles on exactly flat ground: acc is 0 away from them, the distances grow large"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w, 3), 200, np.uint8)
    for _ in range(int(rng.integers(1, 5))):
        bh, bw = int(rng.integers(2, max(3, h // 3 + 1))), int(rng.integers(2, max(3, w // 3 + 1)))
        y, x = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
        img[y:y + bh, x:x + bw] = int(rng.integers(0, 150))
    return img


def patch(h, w, seed):
    """a square of noise (side seed // 1000, generator seed % 1000) in the top left corner of flat ground: distances up to the crop's extent"""
    s = seed // 1000
    img = np.full((h, w, 3), 200, np.uint8)
    img[:s, :s] = np.random.default_rng(seed % 1000).integers(0, 256, (min(h, s), s, 3), dtype=np.uint8)
    return img


def step(h, w, seed):
    """vertical step at column `seed % w`, height of the step 1 + seed // w grey levels above 0: a band of non-zero acc on zero ground"""
    img = np.zeros((h, w, 3), np.uint8)
    img[:, seed % w:] = min(255, 1 + seed // w)
    return img


def const(h, w, seed):
    return np.full((h, w, 3), seed, np.uint8)


def diag(h, w, seed):
    """0 / 255 diagonal step: dx^2 + dy^2 of the unblurred scale is above 2^24"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat(np.where(xx + yy >= seed, 255, 0).astype(np.uint8)[..., None], 3, axis=2)


def strokes(h, w, seed):
    """noise with a few dark strokes, thick enough for their borders to survive the opening"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for _ in range(3):
        if rng.integers(0, 2) and h >= 4:
            y, t = int(rng.integers(0, h)), int(rng.integers(2, 6))
            img[y:y + t, int(rng.integers(0, max(1, w // 2))):] = int(rng.integers(0, 30))
        else:
            x, t = int(rng.integers(0, w)), int(rng.integers(2, 6))
            img[int(rng.integers(0, max(1, h // 2))):, x:x + t] = int(rng.integers(0, 30))
    return img


KINDS = {"noise": noise, "blobs": blobs, "patch": patch, "step": step, "const": const, "diag": diag, "strokes": strokes}

# (kind, h, w, seed): found by a seeded search over these recipes on the CPU (smallest shapes first), one case per category that
# tests/test_dtedge_cases_cpu.py asks for; the categories each case covers are recomputed there, not stored
CASES = [
    ("const", 16, 16, 127),     # every pixel an edge; all three percentiles ties
    ("diag", 24, 24, 24),       # acc.max()^2 > 2^24
    ("noise", 11, 11, 0),       # acc90 mid with frac == 0; no edge survives the opening
    ("noise", 11, 11, 5),       # acc90 top
    ("noise", 9, 9, 1),         # acc90 low
    ("noise", 5, 9, 0),         # acc90 non-tie, frac >= .5
    ("noise", 6, 7, 1),         # acc90 top, frac >= .5, and numpy's two lerp forms round to different float64 there
    ("noise", 48, 70, 0),       # acc90 non-tie, frac < .5
    ("step", 4, 20, 2),         # acc90: key 0.0, successor non-zero
    ("noise", 3, 17, 15),       # dist99 mid, frac >= .5
    ("noise", 9, 9, 0),         # dist99 non-tie, frac < .5
    ("noise", 8, 8, 4),         # dist99 top
    ("patch", 110, 222, 64000),  # dist99 low (two chamfer sums 899 / 65536 apart near 149 px), frac >= .5
    ("patch", 120, 204, 64000),  # dist99 low, frac < .5
    ("noise", 48, 70, 11),      # dist1 top, frac >= .5
    ("noise", 40, 50, 134),     # dist1 top (4 edge pixels)
    ("noise", 45, 52, 40),      # dist1 top, frac < .5
    ("noise", 55, 64, 68),      # dist1 mid, frac < .5
    ("noise", 64, 100, 38),     # dist1 mid, frac >= .5
    ("blobs", 16, 120, 2),      # dist1: key 0.0, successor non-zero
]


def make(case):
    kind, h, w, seed = case
    img = KINDS[kind](h, w, seed)
    assert img.shape == (h, w, 3) and img.dtype == np.uint8
    return img


def case_id(case):
    return "%s-%dx%d-s%d" % case


@functools.lru_cache(maxsize=None)
def oracle_stages(case):
    """(acc, edges, dist, (thr, lo, hi, mn, mx), out) of the CPU oracle: computed once per case, shared, read-only"""
    st = od.stages(make(case))
    for a in (st[0], st[1], st[2], st[4]):
        a.setflags(write=False)
    return st


def classify(values, q):
    """what the q-th percentile of float32 `values` asks of the select: dict(rank, succ, key, nxt (uint32 bit patterns), source, frac)"""
    v = np.ascontiguousarray(values, np.float32).ravel()
    assert not np.signbit(v).any()                      # non-negative floats order as their bit patterns
    bits = np.sort(v.view(np.uint32))
    n = bits.size
    vi = (n - 1) * (q / 100.0)
    rank = int(math.floor(vi))
    succ = min(rank + 1, n - 1)
    key, nxt = int(bits[rank]), int(bits[succ])
    source = "tie" if key == nxt else "low" if key >> 10 == nxt >> 10 else "mid" if key >> 20 == nxt >> 20 else "top"
    # numpy's lerp is a + (b - a) t, replaced by b - (b - a) (1 - t) where t >= 0.5: do the two float64 results differ here?
    a, b = (float(x) for x in np.array([key, nxt], np.uint32).view(np.float32))
    d, t = float(np.float32(b) - np.float32(a)), vi - rank
    return dict(rank=rank, succ=succ, key=key, nxt=nxt, source=source, frac=t, lerp_forms_differ=t >= 0.5 and a + d * t != b - d * (1.0 - t))


def categories(case):
    """the set of coverage labels of one case (see tests/test_dtedge_cases_cpu.py)"""
    acc, edges, dist, _, _ = oracle_stages(case)
    out = set()
    for name, vals, q in (("acc90", acc, 90), ("dist99", dist, 99), ("dist1", dist, 1)):
        c = classify(vals, q)
        out.add("%s:%s" % (name, c["source"]))
        if c["source"] != "tie":
            out.add("%s:%s" % (name, "frac0" if c["frac"] == 0 else "frac<.5" if c["frac"] < 0.5 else "frac>=.5"))
            if c["key"] == 0:
                out.add("%s:zero-key" % name)
            if c["lerp_forms_differ"]:
                out.add("%s:lerp-forms-differ" % name)
    if not edges.any():
        assert float(dist.min()) >= 8191.0
        out.add("no-edge")
    if edges.all():
        out.add("all-edge")
    if float(acc.max()) ** 2 > 2.0 ** 24:
        out.add("acc>2^24")
    return out
