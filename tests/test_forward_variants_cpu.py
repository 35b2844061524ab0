"""The cases of test_gpu_forward_variants.py can fail, and a correct forward passes them (no GPU).

As in test_forward_ref_cpu.py the oracle's own forwards (torch on the CPU: the same rounding model, another summation order) play the
device.  Here at the points that file does not visit: class counts whose head slices are unaligned or partial (nc 1, 13, 15), the 80-wide
class branch (nc 80), and YOLO11s in fp32 (1024-channel model.9.cv2, the qkv permutation of the 4-head C2PSA).  The emulated head goes
through the SAME row layout and slicing as the device's ([64 box | nc class | 1 angle] padded to a multiple of 4 floats,
forward_obs._head_obs), so the three store mistakes an epilogue can make at an unaligned slice are mutations of that row."""
import functools

import numpy as np
import pytest
import torch

import forward_obs as fo
import forward_ref as fr
from oracle.yolo11_obb import Yolo11OBB
from test_forward_ref_cpu import _fails, _hide, _store


@functools.lru_cache(maxsize=None)
def _model(scale, nc, ch):
    return Yolo11OBB(scale, nc=nc, ch=ch, seed=0)


@functools.lru_cache(maxsize=None)
def _taps(scale, nc, ch, h, w, prec):
    m = _model(scale, nc, ch)
    x = np.random.default_rng(h + w + nc).integers(0, 256, (1, h, w, ch), dtype=np.uint8)
    taps = {}
    head = m.forward_raw(x, prec, taps)
    obs = {k: v for k, v in taps.items() if k in fr.graph(m)}
    obs["tile"] = x
    assert sum(n in obs for n in m.convs) == len(m.convs) == 96
    return m, obs, head


CORRECT = [("n", nc, 3, "fp32", 64, 96) for nc in (1, 13, 15, 80)] + [("n", 13, 4, "fp32", 64, 96)] + \
          [("n", nc, 3, p, 64, 96) for nc in (13, 80) for p in ("f16", "bf16")] + [("s", 15, 3, "fp32", 64, 64)]


@pytest.mark.parametrize("scale,nc,ch,prec,h,w", CORRECT, ids=str)
def test_correct_forward_satisfies_every_bound(scale, nc, ch, prec, h, w):
    m, obs, head = _taps(scale, nc, ch, h, w, prec)
    assert m.head_c[1] == max(m.head_ch[0], min(nc, 100)) and head.shape[-1] == fo.head_width(m)
    # the head convs' outputs as the GPU test sees them: out of a padded device row, through forward_obs._head_obs
    row = torch.full(head.shape[:2] + (fo.head_width_padded(m),), float("nan"))
    row[..., :fo.head_width(m)] = head
    via_row = fo._head_obs(m, row, h, w)
    assert sum(via_row[n].shape[1] for n in fr.head_names(0)) == fo.head_width(m)
    for n, t in via_row.items():
        assert torch.equal(t, obs[n].double()), n
    everything = set(m.convs) | {"attn:model.10.m.0.attn", "up:up13", "up:up16"} | {f"pool:model.9.pool{i}" for i in range(3)}
    for form, o in (("single ", obs), ("fused ", _hide(m, obs))):
        o = dict(o, **via_row)
        ev = fr.Evaluator(m, prec, o)
        ratios, covered = fr.check_all(ev, [k for k in o if k != "tile"], label=f"{prec} {scale} nc{nc} ch{ch} {h}x{w} {form}")
        assert covered == everything, everything ^ covered
        assert all(n in ratios for i in range(3) for n in fr.head_names(i))
        print(f"{prec} {scale} nc{nc} ch{ch} {h}x{w} {form}: worst ratio {max(ratios.values()):.3f} at {max(ratios, key=ratios.get)}")


# ---------------------------------------------------------------------------------------------- the head row at an unaligned slice
def _float4s(m, row, fill):
    """the class slice stored as whole float4s after the angle: the lanes past the last class (here: its value again) land in the angle column"""
    nc = m.nc
    row[64 + nc:64 + (nc + 3) // 4 * 4] = row[64 + nc - 1].clone()
    return {"model.23.cv4.{}.2"}


def _angle_one_early(m, row, fill):
    nc = m.nc
    row[64 + nc - 1] = row[64 + nc].clone()
    row[64 + nc] = fill  # never written
    return {"model.23.cv3.{}.2", "model.23.cv4.{}.2"}


def _last_class_unwritten(m, row, fill):
    row[64 + m.nc - 1] = fill
    return {"model.23.cv3.{}.2"}


@pytest.mark.parametrize("fill", [0.0, float("nan")], ids=["zero-filled", "nan-filled"])  # (what the unwritten element holds: torch.zeros, or the guarded buffer's 0xff bytes)
@pytest.mark.parametrize("mutation", [_float4s, _angle_one_early, _last_class_unwritten], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("nc", [13, 15])
def test_head_row_store_mistakes_fail(nc, mutation, fill):
    """one anchor's row mutated, at a border anchor and at an interior anchor of every level: the groups the mistake touches fail, the others pass"""
    h, w = 64, 96
    m, obs, head = _taps("n", nc, 3, h, w, "fp32")
    assert (64 + nc) % 4 != 0 or nc % 4 != 0
    ev = fr.Evaluator(m, "fp32", obs)
    bound = {n: fr.group_bound(ev, n) for i in range(3) for n in fr.head_names(i)}
    good = torch.zeros(head.shape[:2] + (fo.head_width_padded(m),))
    good[..., :fo.head_width(m)] = head
    for n, t in fo._head_obs(m, good, h, w).items():
        fr.check_group(f"nc{nc} {n} emulated, unmutated", t, bound[n][0], bound[n][1])
    off = 0
    for i, s in enumerate((8, 16, 32)):
        H, W = h // s, w // s
        for (y, x) in ((0, 0), (H // 2, W // 2)):
            row = good.clone()
            touched = {t.format(i) for t in mutation(m, row[0, off + y * W + x], fill)}
            for n, t in fo._head_obs(m, row, h, w).items():
                if n in touched:
                    _fails(f"nc{nc} {n} {mutation.__name__} at level {i} ({y}, {x})", t, bound[n][0], bound[n][1])
                else:
                    fr.check_group(f"nc{nc} {n} untouched by {mutation.__name__} at level {i} ({y}, {x})", t, bound[n][0], bound[n][1])
        off += H * W


# ---------------------------------------------------------------------------------------------- s, fp32
S_TILE = (128, 160)  # a 4 x 5 map at stride 32: (0, 0) is a border pixel, (2, 2) an interior one


def _s_pixels(t):
    H, W = t.shape[2:]
    assert H >= 3 and W >= 3
    return [(0, 0), (H // 2, W // 2)]


@pytest.mark.parametrize("section", ["qkv", "k"])
def test_s_qkv_permutation_with_two_heads_swapped_fails(section):
    """the device stores qkv as [q heads | k heads | v heads] (4 heads at s); a packing that swaps heads 1 and 2 -- everywhere, or in the k
    section alone -- is read back through the same un-permutation as the GPU test's and fails the qkv group"""
    m, obs, _ = _taps("s", 12, 3, *S_TILE, "fp32")
    nh, hd = m.psa_heads, m.psa_c // m.psa_heads
    kd = hd // 2
    assert (nh, kd, hd) == (4, 32, 64)
    name = "model.10.m.0.attn.qkv"
    ref, E, _ = fr.group_bound(fr.Evaluator(m, "fp32", obs), name)
    perm = fr.qkv_device_order(nh, kd, hd)
    dev = obs[name][:, perm]  # what a correct device holds
    good = fo.qkv_to_oracle(m, dev)
    assert torch.equal(good, obs[name])
    fr.check_group(f"{name} emulated, unmutated", good, ref, E)
    sw = {1: 2, 2: 1}
    bad_perm = list(perm)
    for c, src in enumerate(perm):
        hh, d = divmod(src, 2 * kd + hd)
        if section == "qkv" or kd <= d < 2 * kd:
            bad_perm[c] = sw.get(hh, hh) * (2 * kd + hd) + d
    assert sorted(bad_perm) == sorted(perm) and bad_perm != perm
    bad = fo.qkv_to_oracle(m, obs[name][:, bad_perm])
    for (y, x) in _s_pixels(ref):
        got = good.clone()
        got[:, :, y, x] = bad[:, :, y, x]
        _fails(f"{name} heads 1 / 2 swapped ({section}) at ({y}, {x})", got, ref, E)


@pytest.mark.parametrize("piece", [0, 37, 63])
def test_s_dropped_16_channel_piece_of_the_1024_channel_conv_fails(piece):
    """model.9.cv2 at s sums 1024 input channels in 16-channel pieces (k_conv_f32): one piece left out of the sum fails the group"""
    m, obs, _ = _taps("s", 12, 3, *S_TILE, "fp32")
    name = "model.9.cv2"
    assert m.convs[name].c1 == 1024

    def drop(w, b):
        w[:, 16 * piece:16 * piece + 16] = 0.0
        return w, b
    ref, E, _ = fr.group_bound(fr.Evaluator(m, "fp32", obs), name)
    good = _store(ref, "fp32", name)
    fr.check_group(f"{name} emulated, unmutated", good, ref, E)
    bad = _store(fr.Evaluator(m, "fp32", obs, mutate={name: drop}).node(name)[0], "fp32", name)
    for (y, x) in _s_pixels(ref):
        got = good.clone()
        got[:, :, y, x] = bad[:, :, y, x]
        _fails(f"{name} without input channels [{16 * piece}, {16 * piece + 16}) at ({y}, {x})", got, ref, E)
