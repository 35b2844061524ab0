"""f1 (training batches): the batch `model.train(...)` (Train_OBB.py:796-841) is fed, built on the device from a pool of tiles.  The reference leaves
every augmentation argument at its Ultralytics default -- 4-image Mosaic with probability 1, RandomPerspective(translate 0.1, scale 0.5, degrees 0),
RandomHSV(0.015, 0.7, 0.4), fliplr 0.5 -- and those rules are restated here from recall (Ultralytics 8.3.x; neither the package nor cv2 is installed,
so parity with them is UNPINNED, like `train.pad_targets` and `train.optimizer_config`; pinned is the device against tests/aug_ref.py).

The host draws the random numbers (`sample_params`: a few hundred bytes per tile); the device does everything that touches a pixel or a label
(`ops.aug_tiles`, `ops.aug_labels`): nothing is read back, so a batch can be captured in a graph and replayed with the table rewritten in place.
Out of scope: mixup, copy-paste, Albumentations, rect batching, file I/O."""
from dataclasses import dataclass, replace

import numpy as np
import torch

from . import _lib, ops

MOSAIC, FLIPLR, FLIPUD, HSV = 1, 2, 4, 8  # OBB_AUG_* of include/obbhip.h

# one record of the parameter table, byte for byte the layout documented in include/obbhip.h
REC = np.dtype([("inv", "<f8", (6,)), ("fwd", "<f8", (6,)), ("scale", "<f8"), ("xc", "<i4"), ("yc", "<i4"), ("src", "<i4", (4,)), ("flags", "<u4"),
                ("reserved", "<i4"), ("lut", "u1", (768,))])
assert REC.itemsize == _lib.AUG_REC_BYTES


@dataclass(frozen=True)
class AugmentConfig:
    """The Ultralytics defaults `model.train(...)` runs with when no augmentation argument is given."""
    mosaic: float = 1.0
    translate: float = 0.1
    scale: float = 0.5
    degrees: float = 0.0
    hsv_h: float = 0.015
    hsv_s: float = 0.7
    hsv_v: float = 0.4
    fliplr: float = 0.5
    flipud: float = 0.0
    # box_candidates (the segment case): both sides above wh_thr px, aspect under ar_thr, area after / before above area_thr
    wh_thr: float = 2.0
    ar_thr: float = 100.0
    area_thr: float = 0.01

    def close_mosaic(self, closed=True):
        """The last epochs of a run (`close_mosaic`): mosaic probability 0, everything else as it is."""
        return replace(self, mosaic=0.0) if closed else self


def hsv_luts(r):
    """RandomHSV's three look-up tables for the gains r = (r_h, r_s, r_v), float64 -> uint8 as numpy casts: [768] = lut_h | lut_s | lut_v"""
    x = np.arange(0, 256, dtype=np.float64)
    return np.concatenate([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)])


def affine(S, s, angle_deg, scale, tx, ty):
    """RandomPerspective.affine_transform with shear and perspective at 0: M = T R C [3,3] float64 from a canvas of side S to an output of side s.
    C moves the canvas centre to the origin, R = cv2.getRotationMatrix2D((0, 0), angle, scale), T translates by (tx, ty) * s."""
    Cm, R, T = np.eye(3), np.eye(3), np.eye(3)
    Cm[0, 2] = Cm[1, 2] = -S / 2
    a = np.deg2rad(angle_deg)
    al, be = scale * np.cos(a), scale * np.sin(a)
    R[0, :2] = al, be
    R[1, :2] = -be, al
    T[0, 2], T[1, 2] = tx * s, ty * s
    return T @ R @ Cm


def make_record(rec, M, scale, s, mosaic=False, centre=(0, 0), src=(0, 0, 0, 0), fliplr=False, flipud=False, hsv_gains=None):
    """Fills one REC record from the forward matrix M [3,3] (the inverse is taken here, in double)."""
    M = np.asarray(M, np.float64)
    rec["fwd"] = M[:2].reshape(6)
    rec["inv"] = np.linalg.inv(M)[:2].reshape(6)
    rec["scale"] = scale
    rec["xc"], rec["yc"] = int(centre[0]), int(centre[1])
    rec["src"] = np.asarray(src, np.int32)
    rec["flags"] = (MOSAIC if mosaic else 0) | (FLIPLR if fliplr else 0) | (FLIPUD if flipud else 0) | (HSV if hsv_gains is not None else 0)
    rec["reserved"] = 0
    rec["lut"] = hsv_luts(hsv_gains) if hsv_gains is not None else 0
    return rec


def sample_params(cfg, B, N, s, rng, indices=None):
    """The host table of one batch: REC [B].  rng: numpy RandomState.  Per tile, in this order of draws: mosaic or not; the three other sources from
    the pool (mosaic only; source 0 is `indices[b]`, drawn from the pool when `indices` is None); the centre xc, yc ~ U(s/2, 3s/2) truncated to int;
    angle ~ U(-degrees, degrees), scale ~ U(1 - scale, 1 + scale), translations ~ U(0.5 - translate, 0.5 + translate); the three HSV gains
    U(-1, 1) * (h, s, v) + 1; flipud, fliplr."""
    if indices is None:
        indices = rng.randint(0, N, size=B)
    indices = np.asarray(indices, np.int64).reshape(-1)
    if len(indices) != B or (len(indices) and (indices.min() < 0 or indices.max() >= N)):
        raise ValueError(f"sample_params: {B} indices inside [0, {N}) expected")
    table = np.zeros(B, REC)
    for b in range(B):
        mosaic = rng.uniform() < cfg.mosaic
        src, centre = [int(indices[b]), 0, 0, 0], (0, 0)
        if mosaic:
            src[1:] = [int(v) for v in rng.randint(0, N, size=3)]
            centre = (int(rng.uniform(s / 2, 3 * s / 2)), int(rng.uniform(s / 2, 3 * s / 2)))
        angle = rng.uniform(-cfg.degrees, cfg.degrees)
        sc = rng.uniform(1 - cfg.scale, 1 + cfg.scale)
        tx, ty = rng.uniform(0.5 - cfg.translate, 0.5 + cfg.translate), rng.uniform(0.5 - cfg.translate, 0.5 + cfg.translate)
        gains = rng.uniform(-1, 1, 3) * [cfg.hsv_h, cfg.hsv_s, cfg.hsv_v] + 1
        ud, lr = rng.uniform() < cfg.flipud, rng.uniform() < cfg.fliplr
        make_record(table[b], affine(2 * s if mosaic else s, s, angle, sc, tx, ty), sc, s, mosaic, centre, src, lr, ud,
                    gains if (cfg.hsv_h or cfg.hsv_s or cfg.hsv_v) else None)
    return table


def check_table(table, N, s):
    """What the kernels can only skip (the table is on the device when they run) is an error here, on the host copy."""
    t = np.asarray(table)
    if t.dtype != REC or t.ndim != 1:
        raise ValueError("augment: the table must be a 1-d array of augment.REC records")
    for b, r in enumerate(t):
        n = 4 if r["flags"] & MOSAIC else 1
        if (r["src"][:n] < 0).any() or (r["src"][:n] >= N).any():
            raise ValueError(f"augment: record {b} names pool tile {r['src'][:n].tolist()} of {N}")
        if n == 4 and not (0 <= r["xc"] <= 2 * s and 0 <= r["yc"] <= 2 * s):
            raise ValueError(f"augment: record {b} has its mosaic centre ({r['xc']}, {r['yc']}) outside [0, {2 * s}]")
    return t


def table_to_device(table, device):
    """REC [B] (host) -> uint8 [B, 904] on the device"""
    return torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).reshape(len(table), REC.itemsize).copy()).to(device)


class TrainBatcher:
    """A pool of equal-sized tiles with their labels on the device, and batches drawn from it.
      pool_tiles uint8 [N,s,s,C], pool_labels float64 [N,Lmax,9] (class + 8 corners normalised to the tile), pool_counts int32 [N]
      .batch(indices, rng) -> (tiles uint8 [B,s,s,C], gt_labels, gt_bboxes, mask_gt) ready for `Net.step`; `count` and `params` keep the true number of
        survivors per tile (device) and the host table of the last batch
      .buffers(B) / .batch_into(table, tiles, gt_labels, gt_bboxes, mask_gt, count, params=None): the same into caller-held buffers; with `params` the
        device table is rewritten IN PLACE first, so a captured batch_into replays with new parameters after `write_table`.
    bgr: channel 0 of the pool is blue (the tiler's crops); swap_rb: hand out RGB, as the net is fed."""

    def __init__(self, pool_tiles, pool_labels, pool_counts, cfg=None, n_cap=64, bgr=True, swap_rb=True):
        self.tiles = ops._chk(pool_tiles, torch.uint8, "pool_tiles")
        self.labels = ops._chk(pool_labels, torch.float64, "pool_labels")
        self.counts = ops._chk(pool_counts, torch.int32, "pool_counts")
        if self.tiles.dim() != 4 or self.tiles.shape[1] != self.tiles.shape[2] or self.tiles.shape[3] not in (3, 4):
            raise ValueError("TrainBatcher: pool_tiles must be [N, s, s, 3 or 4]")
        self.N, self.s = int(self.tiles.shape[0]), int(self.tiles.shape[1])
        if self.labels.dim() != 3 or self.labels.shape[0] != self.N or self.labels.shape[2] != 9 or self.counts.shape != (self.N,):
            raise ValueError("TrainBatcher: pool_labels must be [N, Lmax, 9] and pool_counts [N]")
        self.cfg, self.n_cap, self.bgr, self.swap_rb = cfg or AugmentConfig(), int(n_cap), bool(bgr), bool(swap_rb)
        self.count, self.params = None, None

    @classmethod
    def from_tiler(cls, positives, empty_crops=(), cfg=None, n_cap=64, **kw):
        """positives: `tiler.tile_image`'s dicts (crop + label rows); empty_crops: the crops of the selected empty tiles (uint8 [s,s,C] on the device)"""
        crops = [p["crop"] for p in positives] + list(empty_crops)
        if not crops:
            raise ValueError("TrainBatcher.from_tiler: no tiles")
        rows = [np.asarray(p["labels"], np.float64).reshape(-1, 9) for p in positives] + [np.zeros((0, 9))] * len(empty_crops)
        lmax = max(1, max(len(r) for r in rows))
        lab = np.zeros((len(rows), lmax, 9))
        for i, r in enumerate(rows):
            lab[i, :len(r)] = r
        dev = crops[0].device
        return cls(torch.stack(crops).contiguous(), torch.from_numpy(lab).to(dev), torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev),
                   cfg, n_cap, **kw)

    def buffers(self, B):
        """-> (table, tiles, gt_labels, gt_bboxes, mask_gt, count): device buffers for batch_into"""
        d = self.tiles.device
        return (torch.empty((B, REC.itemsize), dtype=torch.uint8, device=d), torch.empty((B, self.s, self.s, self.tiles.shape[3]), dtype=torch.uint8, device=d),
                torch.empty((B, self.n_cap), dtype=torch.int32, device=d), torch.empty((B, self.n_cap, 5), dtype=torch.float32, device=d),
                torch.empty((B, self.n_cap), dtype=torch.bool, device=d), torch.empty((B,), dtype=torch.int32, device=d))

    def write_table(self, table, params):
        """host REC [B] -> the device table, in place (its address is what a captured batch_into reads)"""
        check_table(params, self.N, self.s)
        table.copy_(table_to_device(params, "cpu"), non_blocking=False)
        return table

    def batch_into(self, table, tiles, gt_labels, gt_bboxes, mask_gt, count, params=None):
        if params is not None:
            self.write_table(table, params)
        c = self.cfg
        ops.aug_tiles(self.tiles, table, self.bgr, self.swap_rb, out=tiles)
        ops.aug_labels(self.labels, self.counts, table, self.s, self.n_cap, c.wh_thr, c.ar_thr, c.area_thr, out=(gt_labels, gt_bboxes, mask_gt, count))
        return tiles, gt_labels, gt_bboxes, mask_gt

    def batch(self, indices, rng, params=None):
        """indices: the pool tiles of this batch (each is source 0 of its output tile); rng: numpy RandomState.  `params`: a host table to use as it is."""
        if params is None:
            params = sample_params(self.cfg, len(indices), self.N, self.s, rng, indices)
        bufs = self.buffers(len(params))
        out = self.batch_into(*bufs, params=params)
        self.count, self.params = bufs[5], params
        return out
