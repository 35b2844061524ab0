"""PyTorch-ROCm custom ops over the C-ABI of libobbhip.so (SURVEY.md section 8(b) "Registration").

Every device entry point of include/obbhip.h is registered with the torch dispatcher as `torch.ops.obbhip.<name>` through
`torch.library.custom_op` (device type "cuda" = HIP on ROCm: there is no CPU implementation, a CPU tensor raises).  The registered
form takes the caller's tensors only -- inputs, and outputs as pre-allocated tensors it mutates -- and launches the hand-written HIP
kernels on torch's CURRENT stream, so the ops compose with torch streams, events and `torch.cuda.graph` capture.  PyTorch supplies
device memory and streams, nothing else; no Triton, no multi-backend dispatch.

The plain functions below (`forward`, `decode_nms`, `merge_detections`, ...) are the convenience layer the rest of the package
uses: they allocate the outputs and call `torch.ops.obbhip.*`.
"""
import ctypes as C
import contextlib
import ctypes as _ct  # (for functions whose own argument is named C)
import os
from typing import List, Optional

import torch

from . import _lib

_ctx = {}
T = torch.Tensor


def ctx(device=None):
    """One library context per device (created lazily)."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    if idx not in _ctx:
        h = C.c_void_p()
        _lib.check(_lib.lib().obb_ctx_create(idx, C.byref(h)))
        _ctx[idx] = h
    return _ctx[idx]


def destroy_contexts():
    for h in _ctx.values():
        _lib.lib().obb_ctx_destroy(h)
    _ctx.clear()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _chk(t, dtype, name):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA/HIP tensor (there is no CPU path)")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")
    return t


def _call(name, c, *args):
    _lib.check(getattr(_lib.lib(), name)(c, *args), c)


def _op(name, mutates):
    return torch.library.custom_op(f"obbhip::{name}", mutates_args=mutates, device_types="cuda")


# ================================================================ registered ops (torch.ops.obbhip.*)
# ---------------------------------------------------------------- S2 polygon IoU (Detect_OBB.py:144-154)
@_op("poly_iou_pairs", ("out",))
def _poly_iou_pairs(a: T, b: T, out: T) -> None:
    _call("obb_poly_iou_pairs", ctx(a.device), _p(a), _p(b), a.shape[0], _p(out), _stream())


@_op("poly_iou_matrix", ("out",))
def _poly_iou_matrix(a: T, cls_a: Optional[T], b: T, cls_b: Optional[T], out: T) -> None:
    _call("obb_poly_iou_matrix", ctx(a.device), _p(a), _p(cls_a), a.shape[0], _p(b), _p(cls_b), b.shape[0], _p(out), _stream())


@_op("points_in_quads", ("out",))
def _points_in_quads(pts: T, cls_p: Optional[T], quads: T, cls_q: Optional[T], out: T) -> None:
    _call("obb_points_in_quads", ctx(pts.device), _p(pts), _p(cls_p), pts.shape[0], _p(quads), _p(cls_q), quads.shape[0], _p(out), _stream())


@_op("build_multich", ("out",))
def _build_multich(bgr: T, out: T) -> None:
    _call("obb_build_multich", ctx(bgr.device), _p(bgr), bgr.shape[0], bgr.shape[1], bgr.shape[2], _p(out), _stream())


@_op("build_multich_stages", ("out", "acc", "edges", "dist", "stats"))
def _build_multich_stages(bgr: T, out: T, acc: T, edges: T, dist: T, stats: T) -> None:
    _call("obb_build_multich_stages", ctx(bgr.device), _p(bgr), bgr.shape[0], bgr.shape[1], bgr.shape[2], _p(out), _p(acc), _p(edges), _p(dist), _p(stats),
          _stream())


# ---------------------------------------------------------------- S3 merge_detections (Detect_OBB.py:176-200)
@_op("sort_desc_stable", ("order",))
def _sort_desc_stable(key: T, order: T) -> None:
    _call("obb_sort_desc_stable", ctx(key.device), _p(key), key.shape[0], _p(order), _stream())


@_op("nms_mask", ("mask",))
def _nms_mask(boxes: T, cls: T, thr: float, mask: T) -> None:
    _call("obb_nms_mask", ctx(boxes.device), _p(boxes), _p(cls), boxes.shape[0], float(thr), _p(mask), _stream())


@_op("nms_reduce", ("keep", "n_keep"))
def _nms_reduce(mask: T, n: int, keep: T, n_keep: T) -> None:
    _call("obb_nms_reduce", ctx(mask.device), _p(mask), n, _p(keep), _p(n_keep), _stream())


@_op("merge_detections", ("order", "keep", "n_keep"))
def _merge_detections(boxes: T, cls: T, conf: T, thr: float, order: T, keep: T, n_keep: T) -> None:
    _call("obb_merge_detections", ctx(boxes.device), _p(boxes), _p(cls), _p(conf), boxes.shape[0], float(thr), _p(order), _p(keep), _p(n_keep), _stream())


@_op("merge_segments", ("order", "keep"))
def _merge_segments(boxes: T, cls: T, conf: T, seg_off: T, thr: float, order: T, keep: T) -> None:
    _call("obb_merge_segments", ctx(boxes.device), _p(boxes), _p(cls), _p(conf), _p(seg_off), seg_off.shape[0] - 1, boxes.shape[0], float(thr), _p(order),
          _p(keep), _stream())


# ---------------------------------------------------------------- S4 consensus (Detect_OBB.py:347-423)
@_op("consensus", ("out_idx", "n_out"))
def _consensus(boxes: T, cls: T, conf: T, offsets: List[int], iou_partner: float, cons_low: float, cons_high: float, out_idx: T, n_out: T) -> None:
    off = (C.c_int64 * len(offsets))(*[int(o) for o in offsets])
    _call("obb_consensus", ctx(boxes.device), _p(boxes), _p(cls), _p(conf), off, len(offsets) - 1, float(iou_partner), float(cons_low), float(cons_high),
          _p(out_idx), _p(n_out), _stream())


# ---------------------------------------------------------------- S5 detect_symbols pieces (Detect_OBB.py:202-266)
@_op("tile_postprocess", ("gboxes", "angle", "inside"))
def _tile_postprocess(local_pts: T, cls: T, det_tile: T, rects: T, margin: int, strike_cls: int, gboxes: T, angle: T, inside: T) -> None:
    _call("obb_tile_postprocess", ctx(local_pts.device), _p(local_pts), _p(cls), _p(det_tile), local_pts.shape[0], _p(rects), rects.shape[0], int(margin),
          int(strike_cls), _p(gboxes), _p(angle), _p(inside), _stream())


@_op("tile_survivors", ("records", "tile_off", "n_records"))
def _tile_survivors(det: T, count: T, lb: Optional[T], tile_ids: T, rects: T, margin: int, strike_cls: int, iou_thr: float, records: T, tile_off: T,
                    n_records: T) -> None:
    _call("obb_tile_survivors", ctx(det.device), _p(det), _p(count), det.shape[0], det.shape[1], _p(lb), _p(tile_ids), _p(rects), int(margin), int(strike_cls),
          float(iou_thr), _p(records), _p(tile_off), _p(n_records), _stream())


@_op("select_kept", ("out_boxes", "out_cls", "out_conf", "out_angle", "n_out"))
def _select_kept(order: T, keep: T, boxes: T, cls: T, conf: T, angle: T, out_boxes: T, out_cls: T, out_conf: T, out_angle: T, n_out: T) -> None:
    _call("obb_select_kept", ctx(order.device), _p(order), _p(keep), order.shape[0], _p(boxes), _p(cls), _p(conf), _p(angle), _p(out_boxes), _p(out_cls),
          _p(out_conf), _p(out_angle), _p(n_out), _stream())


@_op("records_to_dets", ("gboxes", "cls", "conf", "angle"))
def _records_to_dets(records: T, n: int, rects: T, strike_cls: int, gboxes: T, cls: T, conf: T, angle: T) -> None:
    _call("obb_records_to_dets", ctx(records.device), _p(records), int(n), _p(rects), int(strike_cls), _p(gboxes), _p(cls), _p(conf), _p(angle), _stream())


@_op("gather_compact", ("out", "counts"))
def _gather_compact(recv: T, out: T, counts: T) -> None:
    _call("obb_gather_compact", ctx(recv.device), _p(recv), recv.shape[0], recv.shape[1] - 1, _p(out), _p(counts), _stream())


@_op("gather_tiles", ("out",))
def _gather_tiles(image: T, rects: T, tile: int, out: T) -> None:
    H, W, Cc = image.shape
    _call("obb_gather_tiles", ctx(image.device), _p(image), H, W, Cc, _p(rects), rects.shape[0], tile, _p(out), _stream())


@_op("letterbox", ("out",))
def _letterbox(image: T, x: int, y: int, x2: int, y2: int, imgsz: int, out: T) -> None:
    H, W, Cc = image.shape
    _call("obb_letterbox", ctx(image.device), _p(image), H, W, Cc, int(x), int(y), int(x2), int(y2), int(imgsz), _p(out), out.shape[0], out.shape[1], _stream())


# ---------------------------------------------------------------- S1 model (Detect_OBB.py:26, 81-83, 228-231)
@_op("forward", ("head",))
def _forward(tiles: T, head: T) -> None:
    B, h, w, _ = tiles.shape
    _call("obb_forward", ctx(tiles.device), _p(tiles), B, h, w, _p(head), _stream())


@_op("forward_gate", ("head", "cmax"))
def _forward_gate(tiles: T, head: T, cmax: T) -> None:
    B, h, w, _ = tiles.shape
    _call("obb_forward_gate", ctx(tiles.device), _p(tiles), B, h, w, _p(head), _p(cmax), _stream())


@_op("decode", ("pred",))
def _decode(head: T, h: int, w: int, pred: T) -> None:
    _call("obb_decode", ctx(head.device), _p(head), head.shape[0], h, w, _p(pred), _stream())


@_op("decode_nms", ("det", "count"))
def _decode_nms(head: T, h: int, w: int, conf: float, iou: float, max_det: int, det: T, count: T) -> None:
    _call("obb_decode_nms", ctx(head.device), _p(head), head.shape[0], h, w, float(conf), float(iou), int(max_det), _p(det), _p(count), _stream())


@_op("decode_nms_gate", ("det", "count"))
def _decode_nms_gate(head: T, cmax: T, h: int, w: int, conf: float, iou: float, max_det: int, det: T, count: T) -> None:
    _call("obb_decode_nms_gate", ctx(head.device), _p(head), _p(cmax), head.shape[0], h, w, float(conf), float(iou), int(max_det), _p(det), _p(count), _stream())


@_op("decode_nms_full", ("det", "count"))
def _decode_nms_full(head: T, h: int, w: int, conf: float, iou: float, max_det: int, det: T, count: T) -> None:
    _call("obb_decode_nms_full", ctx(head.device), _p(head), head.shape[0], h, w, float(conf), float(iou), int(max_det), _p(det), _p(count), _stream())


@_op("probiou_nms", ("order", "keep"))
def _probiou_nms(boxes: T, scores: T, iou: float, order: T, keep: T) -> None:
    _call("obb_probiou_nms", ctx(boxes.device), _p(boxes), _p(scores), boxes.shape[0], float(iou), _p(order), _p(keep), _stream())


@_op("results", ("xywhr", "pts"))
def _results(det: T, lb: Optional[T], xywhr: T, pts: T) -> None:
    _call("obb_results", ctx(det.device), _p(det), _p(lb), det.shape[0], _p(xywhr), _p(pts), _stream())


@_op("probiou_loss", ("loss", "grad_pred"))
def _probiou_loss(pred: T, target: T, weight: Optional[T], target_scores_sum: float, loss: T, grad_pred: T) -> None:
    _call("obb_probiou_loss", ctx(pred.device), _p(pred), _p(target), _p(weight), pred.shape[0], float(target_scores_sum), _p(loss), _p(grad_pred), _stream())


@_op("tile_labels", ("mask", "out"))
def _tile_labels(labels: T, rects: T, min_fraction: float, mask: T, out: T) -> None:
    _call("obb_tile_labels", ctx(labels.device), _p(labels), labels.shape[0], _p(rects), rects.shape[0], float(min_fraction), _p(mask), _p(out), _stream())


@_op("rotated_tal_assign", ("target_labels", "target_bboxes", "target_scores", "fg_mask", "target_gt_idx"))
def _rotated_tal_assign(pd_scores: T, pd_bboxes: T, anc_points: T, gt_labels: T, gt_bboxes: T, mask_gt: T, topk: int, alpha: float, beta: float,
                        target_labels: T, target_bboxes: T, target_scores: T, fg_mask: T, target_gt_idx: T) -> None:
    bs, na, nc = pd_scores.shape
    _call("obb_rotated_tal_assign", ctx(pd_scores.device), _p(pd_scores), _p(pd_bboxes), _p(anc_points), _p(gt_labels), _p(gt_bboxes), _p(mask_gt), bs, na, nc,
          gt_bboxes.shape[1], int(topk), float(alpha), float(beta), _p(target_labels), _p(target_bboxes), _p(target_scores), _p(fg_mask), _p(target_gt_idx), _stream())


@_op("dfl_loss", ("loss", "grad_pred"))
def _dfl_loss(pred_dist: T, target_ltrb: T, weight: Optional[T], reg_max: int, target_scores_sum: float, loss: T, grad_pred: T) -> None:
    _call("obb_dfl_loss", ctx(pred_dist.device), _p(pred_dist), _p(target_ltrb), _p(weight), target_ltrb.shape[0], int(reg_max), float(target_scores_sum),
          _p(loss), _p(grad_pred), _stream())


@_op("bce_loss", ("loss", "grad_logits"))
def _bce_loss(logits: T, targets: T, target_scores_sum: float, loss: T, grad_logits: T) -> None:
    _call("obb_bce_loss", ctx(logits.device), _p(logits), _p(targets), logits.numel(), float(target_scores_sum), _p(loss), _p(grad_logits), _stream())


@_op("sgd_step", ("param", "momentum_buf"))
def _sgd_step(param: T, grad: T, momentum_buf: T, lr: float, momentum: float, weight_decay: float, nesterov: bool, first_step: bool) -> None:
    _call("obb_sgd_step", ctx(param.device), _p(param), _p(grad), _p(momentum_buf), param.numel(), float(lr), float(momentum), float(weight_decay),
          int(bool(nesterov)), int(bool(first_step)), _stream())


@_op("adamw_step", ("param", "exp_avg", "exp_avg_sq"))
def _adamw_step(param: T, grad: T, exp_avg: T, exp_avg_sq: T, step: int, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float) -> None:
    _call("obb_adamw_step", ctx(param.device), _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), int(step), float(lr), float(beta1), float(beta2),
          float(eps), float(weight_decay), _stream())


@_op("bn_silu_fwd", ("running_mean", "running_var", "mean", "invstd", "a"))
def _bn_silu_fwd(z: T, gamma: T, beta: T, eps: float, momentum: float, running_mean: T, running_var: T, mean: T, invstd: T, a: T) -> None:
    C = z.shape[-1]
    _call("obb_bn_silu_fwd_bf16", ctx(z.device), _p(z), z.numel() // C, C, _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean), _p(running_var),
          _p(mean), _p(invstd), _p(a), _stream())


@_op("bn_silu_bwd", ("dgamma", "dbeta", "dz"))
def _bn_silu_bwd(z: T, da: T, gamma: T, beta: T, mean: T, invstd: T, dgamma: T, dbeta: T, dz: T) -> None:
    C = z.shape[-1]
    _call("obb_bn_silu_bwd_bf16", ctx(z.device), _p(z), _p(da), z.numel() // C, C, _p(gamma), _p(beta), _p(mean), _p(invstd), _p(dgamma), _p(dbeta), _p(dz),
          _stream())


@_op("sppf_pools_fwd", ("cat",))
def _sppf_pools_fwd(x: T, cat: T) -> None:
    B, H, W, C = x.shape
    _call("obb_sppf_pools_fwd_bf16", ctx(x.device), _p(x), B, H, W, C, _p(cat), _stream())


@_op("sppf_pools_bwd", ("dx",))
def _sppf_pools_bwd(cat: T, dcat: T, dx: T) -> None:
    B, H, W, C = dx.shape
    _call("obb_sppf_pools_bwd_bf16", ctx(cat.device), _p(cat), _p(dcat), B, H, W, C, _p(dx), _stream())


@_op("upcat_fwd", ("out",))
def _upcat_fwd(a: T, b: T, up: int, out: T) -> None:
    B, H, W, Ca = a.shape
    _call("obb_upcat_fwd_bf16", ctx(a.device), _p(a), _p(b), B, H, W, Ca, b.shape[-1], int(up), _p(out), _stream())


@_op("upcat_bwd", ("da", "db"))
def _upcat_bwd(dout: T, H: int, W: int, Ca: int, up: int, da: Optional[T], db: Optional[T], accum_a: bool, accum_b: bool) -> None:
    _call("obb_upcat_bwd_bf16", ctx(dout.device), _p(dout), dout.shape[0], int(H), int(W), int(Ca), dout.shape[-1] - int(Ca), int(up), _p(da), _p(db),
          int(accum_a), int(accum_b), _stream())


@_op("dwconv3_fwd", ("z",))
def _dwconv3_fwd(x: T, w: T, z: T) -> None:
    B, H, W, C = x.shape
    _call("obb_dwconv3_fwd_bf16", ctx(x.device), _p(x), _p(w), B, H, W, C, _p(z), _stream())


@_op("dwconv3_bwd", ("dx", "dw"))
def _dwconv3_bwd(x: T, dz: T, w: T, dx: Optional[T], dw: Optional[T]) -> None:
    B, H, W, C = dz.shape
    _call("obb_dwconv3_bwd_bf16", ctx(dz.device), _p(x), _p(dz), _p(w), B, H, W, C, _p(dx), _p(dw), _stream())


@_op("headconv_fwd", ("y",))
def _headconv_fwd(x: T, w: T, bias: Optional[T], y: T) -> None:
    cout, cin = w.shape
    _call("obb_headconv_fwd_bf16", ctx(x.device), _p(x), _p(w), _p(bias), x.numel() // cin, cin, cout, _p(y), _stream())


@_op("headconv_bwd", ("dx", "dw", "db"))
def _headconv_bwd(x: T, dy: T, w: T, dx: Optional[T], dw: Optional[T], db: Optional[T]) -> None:
    cout, cin = w.shape
    _call("obb_headconv_bwd_bf16", ctx(dy.device), _p(x), _p(dy), _p(w), dy.numel() // cout, cin, cout, _p(dx), _p(dw), _p(db), _stream())


@_op("stemconv_fwd", ("z",))
def _stemconv_fwd(x: T, w: T, z: T) -> None:
    B, H, W, cin = x.shape
    _call("obb_stemconv_fwd_u8", ctx(x.device), _p(x), _p(w), B, H, W, cin, w.shape[0], _p(z), _stream())


@_op("stemconv_wgrad", ("dw",))
def _stemconv_wgrad(x: T, dz: T, dw: T) -> None:
    B, H, W, cin = x.shape
    _call("obb_stemconv_wgrad_u8", ctx(x.device), _p(x), _p(dz), B, H, W, cin, dz.shape[-1], _p(dw), _stream())


@_op("bn_fwd", ("running_mean", "running_var", "mean", "invstd", "a"))
def _bn_fwd(z: T, gamma: T, beta: T, eps: float, momentum: float, running_mean: T, running_var: T, mean: T, invstd: T, a: T, act: bool) -> None:
    C = z.shape[-1]
    _call("obb_bn_fwd_bf16", ctx(z.device), _p(z), z.numel() // C, C, _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean), _p(running_var),
          _p(mean), _p(invstd), _p(a), int(bool(act)), _stream())


@_op("bn_bwd", ("dgamma", "dbeta", "dz"))
def _bn_bwd(z: T, da: T, gamma: T, beta: T, mean: T, invstd: T, dgamma: T, dbeta: T, dz: T, act: bool) -> None:
    C = z.shape[-1]
    _call("obb_bn_bwd_bf16", ctx(z.device), _p(z), _p(da), z.numel() // C, C, _p(gamma), _p(beta), _p(mean), _p(invstd), _p(dgamma), _p(dbeta), _p(dz),
          int(bool(act)), _stream())


@_op("attn_fwd", ("out", "lse"))
def _attn_fwd(qkv: T, nh: int, out: T, lse: T) -> None:
    B, N = qkv.shape[0], qkv.numel() // (qkv.shape[0] * qkv.shape[-1])
    _call("obb_attn_fwd_bf16", ctx(qkv.device), _p(qkv), B, N, int(nh), _p(out), _p(lse), _stream())


@_op("attn_bwd", ("dqkv",))
def _attn_bwd(qkv: T, out: T, lse: T, dout: T, dv_add: Optional[T], nh: int, dqkv: T) -> None:
    B, N = qkv.shape[0], qkv.numel() // (qkv.shape[0] * qkv.shape[-1])
    _call("obb_attn_bwd_bf16", ctx(qkv.device), _p(qkv), _p(out), _p(lse), _p(dout), _p(dv_add), B, N, int(nh), _p(dqkv), _stream())


@_op("add_bf16", ("out",))
def _add_bf16(a: T, b: T, out: T) -> None:
    _call("obb_add_bf16", ctx(a.device), _p(a), _p(b), a.numel(), _p(out), _stream())


@_op("chanwin", ("dst",))
def _chanwin(src: T, s0: int, add: Optional[T], a0: int, n: int, dst: T, d0: int) -> None:
    _call("obb_chanwin_bf16", ctx(src.device), _p(src), src.shape[-1], int(s0), _p(add), add.shape[-1] if add is not None else 0, int(a0),
          src.numel() // src.shape[-1], int(n), _p(dst), dst.shape[-1], int(d0), _stream())


@_op("conv_pack_multi", ("out",))
def _conv_pack_multi(flat: T, table: T, nrec: int, out: T) -> None:
    _call("obb_conv_pack_multi_bf16", ctx(flat.device), _p(flat), flat.numel(), _p(table), table.numel(), int(nrec), _p(out), out.numel(), _stream())


def _crit_levels(box, cls, angle):
    """-> the host-side level arrays of obb_crit_*: (box[3], box_bf16, cls[3], angle[3], H[3], W[3], B, nc)"""
    vp = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    H = (C.c_int32 * 3)(*[t.shape[1] for t in box])
    W = (C.c_int32 * 3)(*[t.shape[2] for t in box])
    return vp(box), int(box[0].dtype == torch.bfloat16), vp(cls), vp(angle), H, W, box[0].shape[0], cls[0].shape[-1]


@_op("crit_decode", ("pd_scores", "pd_bboxes", "anc_points", "stride"))
def _crit_decode(box0: T, box1: T, box2: T, cls0: T, cls1: T, cls2: T, angle0: T, angle1: T, angle2: T, pd_scores: T, pd_bboxes: T, anc_points: T,
                 stride: T) -> None:
    lv = _crit_levels((box0, box1, box2), (cls0, cls1, cls2), (angle0, angle1, angle2))
    _call("obb_crit_decode", ctx(box0.device), *lv, _p(pd_scores), _p(pd_bboxes), _p(anc_points), _p(stride), _stream())


@_op("crit_loss", ("d_box0", "d_box1", "d_box2", "d_cls0", "d_cls1", "d_cls2", "d_angle0", "d_angle1", "d_angle2", "items", "tss"))
def _crit_loss(box0: T, box1: T, box2: T, cls0: T, cls1: T, cls2: T, angle0: T, angle1: T, angle2: T, target_bboxes: T, target_scores: T, fg_mask: T,
               g_box: float, g_cls: float, g_dfl: float, d_box0: T, d_box1: T, d_box2: T, d_cls0: T, d_cls1: T, d_cls2: T, d_angle0: T, d_angle1: T,
               d_angle2: T, items: T, tss: T) -> None:
    lv = _crit_levels((box0, box1, box2), (cls0, cls1, cls2), (angle0, angle1, angle2))
    vp = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    _call("obb_crit_loss", ctx(box0.device), *lv, _p(target_bboxes), _p(target_scores), _p(fg_mask), (C.c_float * 3)(g_box, g_cls, g_dfl),
          vp((d_box0, d_box1, d_box2)), vp((d_cls0, d_cls1, d_cls2)), vp((d_angle0, d_angle1, d_angle2)), _p(items), _p(tss), _stream())


# ---------------------------------------------------------------- trainer update over flat segments (csrc/trainupd.hip)
def _segs(*lists):
    """-> the host-side segment arrays of obb_*_multi and friends: one void*[nseg] per list of flat tensors, then n int64[nseg] and nseg"""
    k = len(lists[0])
    vp = lambda ts: (C.c_void_p * k)(*[t.data_ptr() if t.numel() else 0 for t in ts])
    return (*[vp(ts) for ts in lists], (C.c_int64 * k)(*[t.numel() for t in lists[0]]), k)


def _floats(v):
    return (C.c_float * len(v))(*[float(x) for x in v])


@_op("grad_sumsq", ("partials",))
def _grad_sumsq(grads: List[T], partials: T) -> None:
    g, n, k = _segs(grads)
    _call("obb_grad_sumsq", ctx(partials.device), g, n, k, _p(partials), partials.numel(), _stream())


@_op("clip_coef", ("clip",))
def _clip_coef(partials: T, max_norm: float, clip: T) -> None:
    _call("obb_clip_coef", ctx(clip.device), _p(partials), partials.numel(), float(max_norm), _p(clip), _stream())


@_op("sgd_step_multi", ("params", "momentum_bufs"))
def _sgd_step_multi(params: List[T], grads: List[T], momentum_bufs: List[T], lrs: List[float], weight_decays: List[float], momentum: float, nesterov: bool,
                    first_step: bool, clip: Optional[T]) -> None:
    p, g, b, n, k = _segs(params, grads, momentum_bufs)
    _call("obb_sgd_step_multi", ctx(params[0].device), p, g, b, n, _floats(lrs), _floats(weight_decays), k, float(momentum), int(bool(nesterov)),
          int(bool(first_step)), _p(clip), _stream())


@_op("adamw_step_multi", ("params", "exp_avgs", "exp_avg_sqs"))
def _adamw_step_multi(params: List[T], grads: List[T], exp_avgs: List[T], exp_avg_sqs: List[T], lrs: List[float], weight_decays: List[float], step: int,
                      beta1: float, beta2: float, eps: float, clip: Optional[T]) -> None:
    p, g, m, v, n, k = _segs(params, grads, exp_avgs, exp_avg_sqs)
    _call("obb_adamw_step_multi", ctx(params[0].device), p, g, m, v, n, _floats(lrs), _floats(weight_decays), k, int(step), float(beta1), float(beta2),
          float(eps), _p(clip), _stream())


@_op("grad_accumulate", ("accs",))
def _grad_accumulate(accs: List[T], grads: List[T], first: bool) -> None:
    a, g, n, k = _segs(accs, grads)
    _call("obb_grad_accumulate", ctx(accs[0].device), a, g, n, k, int(bool(first)), _stream())


@_op("ema_update", ("emas",))
def _ema_update(emas: List[T], srcs: List[T], decay: float) -> None:
    e, s, n, k = _segs(emas, srcs)
    _call("obb_ema_update", ctx(emas[0].device), e, s, n, k, float(decay), _stream())


# ---------------------------------------------------------------- f1 (training batches): augmentation (augment.py)
@_op("aug_tiles", ("out",))
def _aug_tiles(pool: T, table: T, bgr: bool, swap_rb: bool, out: T) -> None:
    N, s, _, Cc = pool.shape
    _call("obb_aug_tiles", ctx(pool.device), _p(pool), N, s, Cc, _p(table), table.shape[0], int(bool(bgr)), int(bool(swap_rb)), _p(out), _stream())


@_op("aug_labels", ("gt_labels", "gt_bboxes", "mask_gt", "count"))
def _aug_labels(pool_labels: T, pool_counts: T, table: T, s: int, wh_thr: float, ar_thr: float, area_thr: float, gt_labels: T, gt_bboxes: T, mask_gt: T,
                count: T) -> None:
    N, Lmax, _ = pool_labels.shape
    _call("obb_aug_labels", ctx(pool_labels.device), _p(pool_labels), _p(pool_counts), N, Lmax, _p(table), table.shape[0], int(s), float(wh_thr), float(ar_thr),
          float(area_thr), gt_labels.shape[1], _p(gt_labels), _p(gt_bboxes), _p(mask_gt), _p(count), _stream())


@_op("fold_blob", ("out",))
def _fold_blob(w_flat: T, g_flat: T, b_flat: T, buffers: T, table: T, nrec: int, eps: float, out: T) -> None:
    _call("obb_fold_blob_f32", ctx(w_flat.device), _p(w_flat), _p(g_flat), _p(b_flat), _p(buffers), _p(table), table.numel(), int(nrec), float(eps), _p(out),
          out.numel(), _stream())


@_op("val_match", ("tp", "best_iou", "best_gt"))
def _val_match(det: T, count: T, gt_labels: T, gt_bboxes: T, mask_gt: T, nc: int, thr: T, tp: T, best_iou: T, best_gt: T) -> None:
    _call("obb_val_match", ctx(det.device), _p(det), _p(count), _p(gt_labels), _p(gt_bboxes), _p(mask_gt), det.shape[0], det.shape[1], gt_labels.shape[1],
          int(nc), _p(thr), thr.numel(), _p(tp), _p(best_iou), _p(best_gt), _stream())


@_op("val_crit_decode", ("pd_scores", "pd_bboxes", "anc_points", "stride"))
def _val_crit_decode(head: T, h: int, w: int, nc: int, pd_scores: T, pd_bboxes: T, anc_points: T, stride: T) -> None:
    _call("obb_val_crit_decode", ctx(head.device), _p(head), head.shape[0], int(h), int(w), int(nc), _p(pd_scores), _p(pd_bboxes), _p(anc_points), _p(stride),
          _stream())


@_op("val_crit_items", ("items", "tss"))
def _val_crit_items(head: T, h: int, w: int, nc: int, target_bboxes: T, target_scores: T, fg_mask: T, g_box: float, g_cls: float, g_dfl: float, items: T,
                    tss: T, accumulate: bool) -> None:
    _call("obb_val_crit_items", ctx(head.device), _p(head), head.shape[0], int(h), int(w), int(nc), _p(target_bboxes), _p(target_scores), _p(fg_mask),
          (C.c_float * 3)(g_box, g_cls, g_dfl), _p(items), _p(tss), int(bool(accumulate)), _stream())


@_op("val_confusion", ("matrix",))
def _val_confusion(det: T, count: T, gt_labels: T, gt_bboxes: T, mask_gt: T, nc: int, conf_thr: float, iou_thr: float, matrix: T) -> None:
    _call("obb_val_confusion", ctx(det.device), _p(det), _p(count), _p(gt_labels), _p(gt_bboxes), _p(mask_gt), det.shape[0], det.shape[1], gt_labels.shape[1],
          int(nc), float(conf_thr), float(iou_thr), _p(matrix), _stream())


@_op("debug_activation", ("out",))
def _debug_activation(name: str, B: int, h: int, w: int, out: T) -> None:
    n = C.c_int64(0)
    shp = (C.c_int32 * 3)()
    _call("obb_debug_activation", ctx(out.device), h, w, B, name.encode(), _p(out), out.numel(), C.byref(n), shp, _stream())


_O = torch.ops.obbhip


# ================================================================ convenience layer (allocates the outputs)
def poly_iou_pairs(a, b):
    """a, b: [M,8] float64 -> [M] float64   (compute_polygon_iou per row, Detect_OBB.py:144)"""
    a = _chk(a, torch.float64, "a").reshape(-1, 8)
    b = _chk(b, torch.float64, "b").reshape(-1, 8)
    if a.shape != b.shape:
        raise ValueError("poly_iou_pairs: shape mismatch")
    out = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
    _O.poly_iou_pairs(a, b, out)
    return out


def poly_iou_matrix(a, b, cls_a=None, cls_b=None):
    a = _chk(a, torch.float64, "a").reshape(-1, 8)
    b = _chk(b, torch.float64, "b").reshape(-1, 8)
    if cls_a is not None:
        _chk(cls_a, torch.int32, "cls_a")
        _chk(cls_b, torch.int32, "cls_b")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float64, device=a.device)
    _O.poly_iou_matrix(a, cls_a, b, cls_b, out)
    return out


def build_multich(bgr_tiles, out=None):
    """uint8 [B,h,w,3] BGR crops -> uint8 [B,h,w,4] = RGB + distance-transform edge channel (Detect_OBB.py:87-133)"""
    t = _chk(bgr_tiles, torch.uint8, "bgr_tiles")
    assert t.dim() == 4 and t.shape[3] == 3
    if out is None:
        out = torch.empty((t.shape[0], t.shape[1], t.shape[2], 4), dtype=torch.uint8, device=t.device)
    else:
        _chk(out, torch.uint8, "out")
        assert tuple(out.shape) == (t.shape[0], t.shape[1], t.shape[2], 4)
    _O.build_multich(t, out)
    return out


def build_multich_stages(bgr_tiles):
    """build_multich with its intermediates read out: -> (out uint8 [B,h,w,4], acc float32 [B,h,w], edges uint8 [B,h,w] after the opening,
    dist float32 [B,h,w], stats float64 [B,5] = thr, lo, hi, mn, mx).  The same launches as build_multich, then dense copies."""
    t = _chk(bgr_tiles, torch.uint8, "bgr_tiles")
    assert t.dim() == 4 and t.shape[3] == 3
    B, h, w = t.shape[:3]
    out = torch.empty((B, h, w, 4), dtype=torch.uint8, device=t.device)
    acc = torch.empty((B, h, w), dtype=torch.float32, device=t.device)
    edges = torch.empty((B, h, w), dtype=torch.uint8, device=t.device)
    dist = torch.empty((B, h, w), dtype=torch.float32, device=t.device)
    stats = torch.empty((B, 5), dtype=torch.float64, device=t.device)
    _O.build_multich_stages(t, out, acc, edges, dist, stats)
    return out, acc, edges, dist, stats


def points_in_quads(pts, quads, cls_p=None, cls_q=None):
    """[np, nq] uint8: point i strictly inside the valid quad j (same class when both class vectors are given)"""
    pts = _chk(pts, torch.float64, "pts").reshape(-1, 2)
    quads = _chk(quads, torch.float64, "quads").reshape(-1, 8)
    if cls_p is not None:
        _chk(cls_p, torch.int32, "cls_p")
        _chk(cls_q, torch.int32, "cls_q")
    out = torch.zeros((pts.shape[0], quads.shape[0]), dtype=torch.uint8, device=pts.device)
    _O.points_in_quads(pts, cls_p, quads, cls_q, out)
    return out


def sort_desc_stable(key):
    key = _chk(key, torch.float64, "key")
    order = torch.empty(key.shape[0], dtype=torch.int32, device=key.device)
    _O.sort_desc_stable(key, order)
    return order


def nms_mask(boxes_sorted, cls_sorted, thr):
    b = _chk(boxes_sorted, torch.float64, "boxes").reshape(-1, 8)
    c = _chk(cls_sorted, torch.int32, "cls")
    n = b.shape[0]
    w = (n + 63) // 64
    mask = torch.zeros((w, max(n, 1)), dtype=torch.int64, device=b.device)
    _O.nms_mask(b, c, float(thr), mask)
    return mask


def nms_reduce(mask, n):
    keep = torch.zeros(n, dtype=torch.uint8, device=mask.device)
    nk = torch.zeros(1, dtype=torch.int32, device=mask.device)
    _O.nms_reduce(mask, n, keep, nk)
    return keep, nk


def merge_detections(boxes, cls, conf, thr):
    """-> (order int32[n]: sorted position -> input row, keep uint8[n] in sorted order, n_keep int32[1])"""
    b = _chk(boxes, torch.float64, "boxes").reshape(-1, 8)
    c = _chk(cls, torch.int32, "cls")
    s = _chk(conf, torch.float64, "conf")
    n = b.shape[0]
    order = torch.empty(n, dtype=torch.int32, device=b.device)
    keep = torch.empty(n, dtype=torch.uint8, device=b.device)  # (every position is written by the library)
    nk = torch.empty(1, dtype=torch.int32, device=b.device)
    _O.merge_detections(b, c, s, float(thr), order, keep, nk)
    return order, keep, nk


def merge_segments(boxes, cls, conf, seg_off, thr):
    """Batched per-tile merge (Detect_OBB.py:264).  seg_off int32[nseg+1] device.  Segments of any length (the library takes long
    ones through its dense path)."""
    b = _chk(boxes, torch.float64, "boxes").reshape(-1, 8)
    c = _chk(cls, torch.int32, "cls")
    s = _chk(conf, torch.float64, "conf")
    so = _chk(seg_off, torch.int32, "seg_off")
    n = b.shape[0]
    order = torch.empty(n, dtype=torch.int32, device=b.device)
    keep = torch.zeros(n, dtype=torch.uint8, device=b.device)
    _O.merge_segments(b, c, s, so, float(thr), order, keep)
    return order, keep


def consensus(boxes, cls, conf, offsets, iou_partner=0.40, cons_low=0.25, cons_high=0.70):
    b = _chk(boxes, torch.float64, "boxes").reshape(-1, 8)
    c = _chk(cls, torch.int32, "cls")
    s = _chk(conf, torch.float64, "conf")
    out = torch.empty(max(1, b.shape[0]), dtype=torch.int32, device=b.device)
    nout = torch.zeros(1, dtype=torch.int32, device=b.device)
    _O.consensus(b, c, s, [int(o) for o in offsets], float(iou_partner), float(cons_low), float(cons_high), out, nout)
    return out, nout


def tile_grid(H, W, tile, overlap):
    """Host helper -> int32 numpy [ntiles,4] (x, y, x2, y2) in reference visiting order."""
    import numpy as np
    n = C.c_int64(0)
    _lib.check(_lib.lib().obb_tile_grid(H, W, tile, overlap, None, 0, C.byref(n)))
    rects = np.zeros((max(1, n.value), 4), np.int32)
    _lib.check(_lib.lib().obb_tile_grid(H, W, tile, overlap, rects.ctypes.data_as(_lib.c_ip), n.value, C.byref(n)))
    return rects[:n.value]


def tile_postprocess(local_pts, cls, det_tile, rects, margin, strike_cls=1):
    lp = _chk(local_pts, torch.float32, "local_pts").reshape(-1, 8)
    c = _chk(cls, torch.int32, "cls")
    dt = _chk(det_tile, torch.int32, "det_tile")
    r = _chk(rects, torch.int32, "rects").reshape(-1, 4)
    n = lp.shape[0]
    gb = torch.empty((n, 8), dtype=torch.float64, device=lp.device)
    ang = torch.empty(n, dtype=torch.float64, device=lp.device)
    ins = torch.empty(n, dtype=torch.uint8, device=lp.device)
    _O.tile_postprocess(lp, c, dt, r, int(margin), int(strike_cls), gb, ang, ins)
    return gb, ang, ins


def rotated_tal_assign(pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt, topk=10, alpha=0.5, beta=6.0):
    """RotatedTaskAlignedAssigner.forward -> (target_labels int32[bs,na], target_bboxes f32[bs,na,5], target_scores f32[bs,na,nc], fg_mask bool[bs,na],
    target_gt_idx int32[bs,na]); inputs as in ultralytics (pd_scores sigmoid probabilities [bs,na,nc], boxes xywhr in pixels, gt_labels [bs,n_max(,1)],
    mask_gt [bs,n_max(,1)])."""
    ps = _chk(pd_scores.float().contiguous(), torch.float32, "pd_scores")
    pb = _chk(pd_bboxes.float().contiguous(), torch.float32, "pd_bboxes")
    ap = _chk(anc_points.float().contiguous(), torch.float32, "anc_points")
    bs, na, nc = ps.shape
    gb = gt_bboxes.float().contiguous()
    n_max = gb.shape[1]
    gl = gt_labels.reshape(bs, n_max).to(torch.int32).contiguous()
    mg = mask_gt.reshape(bs, n_max).to(torch.uint8).contiguous()
    d = ps.device
    tl = torch.empty((bs, na), dtype=torch.int32, device=d)
    tb = torch.empty((bs, na, 5), dtype=torch.float32, device=d)
    ts = torch.empty((bs, na, nc), dtype=torch.float32, device=d)
    fg = torch.empty((bs, na), dtype=torch.uint8, device=d)
    ti = torch.empty((bs, na), dtype=torch.int32, device=d)
    _O.rotated_tal_assign(ps, pb, ap, gl, gb, mg, int(topk), float(alpha), float(beta), tl, tb, ts, fg, ti)
    return tl, tb, ts, fg.bool(), ti


def conv_dgrad_bf16(dy, weight):
    """dy bf16 [B,H,W,cout] (device, NHWC), weight fp32 [cout,cin,k,k] (any device; repacked on the host per call) -> dx bf16 [B,H,W,cin]: the
    input gradient of the stride-1 `same` convolution, on the forward's bf16 MFMA kernel with flipped / transposed weights."""
    d = _chk(dy, torch.bfloat16, "dy")
    B, H, W, cout = d.shape
    w = weight.detach().float().cpu().contiguous()
    assert w.shape[0] == cout and w.shape[2] == w.shape[3] and w.shape[2] in (1, 3)
    cin, ks = int(w.shape[1]), int(w.shape[2])
    dx = torch.empty((B, H, W, cin), dtype=torch.bfloat16, device=d.device)
    _call("obb_conv_dgrad_bf16", ctx(d.device), _p(d), w.numpy().ctypes.data_as(_lib.c_fp), B, H, W, cin, cout, ks, _p(dx), _stream())
    return dx


def _stride_ok(ks, stride):
    if stride not in (1, 2) or (stride == 2 and ks != 3):
        raise ValueError(f"stride {stride} with k = {ks}: stride 1 (k 1 or 3) and stride 2 (k 3) are built")


def _conv_wgrad(fn, x, dy, ks, stride, out):
    """The body of conv_wgrad_bf16 / conv_wgrad_c8_bf16 (`fn`: the public name): the C entry points differ in the channel counts they accept."""
    _stride_ok(ks, stride)
    xx, d = _chk(x, torch.bfloat16, "x"), _chk(dy, torch.bfloat16, "dy")
    B, H, W, cin = xx.shape
    cout = d.shape[3]
    if tuple(d.shape[:3]) != (B, (H + stride - 1) // stride, (W + stride - 1) // stride):
        raise ValueError(f"{fn}: dy {tuple(d.shape)} does not match x {tuple(xx.shape)} at stride {stride}")
    dw = torch.empty((cout, cin, ks, ks), dtype=torch.float32, device=xx.device) if out is None else _chk(out, torch.float32, "out")
    if dw.shape != (cout, cin, ks, ks):
        raise ValueError(f"{fn}: out has the wrong shape")
    if fn == "conv_wgrad_c8_bf16":
        _call("obb_conv_wgrad_c8_bf16", ctx(xx.device), _p(xx), _p(d), B, H, W, cin, cout, int(ks), int(stride), _p(dw), _stream())
    elif stride == 2:
        _call("obb_conv_wgrad_s2_bf16", ctx(xx.device), _p(xx), _p(d), B, H, W, cin, cout, _p(dw), _stream())
    else:
        _call("obb_conv_wgrad_bf16", ctx(xx.device), _p(xx), _p(d), B, H, W, cin, cout, int(ks), _p(dw), _stream())
    return dw


def conv_wgrad_bf16(x, dy, ks, stride=1, out=None):
    """x bf16 [B,H,W,cin], dy bf16 [B,Ho,Wo,cout] (NHWC, device) -> dw fp32 [cout,cin,ks,ks] (into `out` if given): the weight gradient of the
    `same`-padded convolution (stride 1: Ho = H; stride 2, k 3: Ho = (H + 1) // 2), fp32 accumulation, deterministic.  Channel counts in
    multiples of 64; anything else is refused."""
    return _conv_wgrad("conv_wgrad_bf16", x, dy, ks, stride, out)


def conv_wgrad_c8_bf16(x, dy, ks, stride=1, out=None):
    """conv_wgrad_bf16 for channel counts that are multiples of 8 (both at least 8), not only of 64: the same kernel behind another check, so at
    multiples of 64 the two give the same bits."""
    return _conv_wgrad("conv_wgrad_c8_bf16", x, dy, ks, stride, out)


def _packed_elems(device, cout, cin, ks, H, W, stride, dgrad_form):
    """Elements of the packed weights of a conv layer on H x W input maps: the stride-2 forward form has a layout (and a query) of its own."""
    n = C.c_int64(0)
    if stride == 2 and not dgrad_form:
        _call("obb_conv_s2_packed_elems", ctx(device), cout, cin, int(H), int(W), C.byref(n))
    else:
        _call("obb_conv_packed_elems", ctx(device), cout, cin, ks, int(H), int(W), int(bool(dgrad_form)), C.byref(n))
    return n.value


def conv_pack_bf16(w, H, W, dgrad_form=False, stride=1):
    """fp32 OIHW master weights (device) -> the bf16 MFMA fragment order of the conv kernel for H x W input maps, packed ON THE DEVICE (no
    host repack, no synchronisation); dgrad_form: the flipped / channel-transposed weights whose forward convolution is the input gradient.
    The dgrad form does not depend on the stride: the stride-2 input gradient (conv_dgrad_s2_bf16) is a stride-1 conv on the H x W map."""
    ww = _chk(w, torch.float32, "w")
    cout, cin, ks, _ = ww.shape
    _stride_ok(ks, stride)
    out = torch.empty(_packed_elems(ww.device, cout, cin, ks, H, W, stride, dgrad_form), dtype=torch.bfloat16, device=ww.device)
    if stride == 2 and not dgrad_form:
        _call("obb_conv_s2_pack_bf16", ctx(ww.device), _p(ww), cout, cin, int(H), int(W), _p(out), _stream())
    else:
        _call("obb_conv_pack_bf16", ctx(ww.device), _p(ww), cout, cin, ks, int(H), int(W), int(bool(dgrad_form)), _p(out), _stream())
    return out


class PackTable:
    """What `conv_pack_plan` returns: `table` (int64 device tensor: the records of csrc/convgrad.hip's k_pack_conv_multi_bf16), `layers` (the
    tuples it was planned from), `dst_off` / `n_elems` (per record: its segment of the packed buffer), `total` (elements of the packed buffer) and
    `src_elems` (elements of the flat weight buffer)."""

    def __init__(self, table, layers, dst_off, n_elems, total, src_elems):
        self.table, self.layers, self.dst_off, self.n_elems, self.total, self.src_elems = table, layers, dst_off, n_elems, total, src_elems

    nrec = property(lambda self: len(self.layers))


def conv_pack_plan(device, layers, src_elems):
    """The plan of `conv_pack_multi_bf16`, made ONCE per (layer list, input size): layers = [(cout, cin, ks, stride, H, W, dgrad_form, src_off)],
    H x W the layer's INPUT map and src_off the element offset of its [cout,cin,ks,ks] fp32 weights in a flat buffer of src_elems elements -> a
    `PackTable`.  Each record is planned as `conv_pack_bf16` plans the same layer (stride 2 in the forward form: the s2 layout; the dgrad form does
    not depend on the stride), and its segment starts at a multiple of 256 elements.  Synchronises (the table is copied to the device)."""
    layers = [tuple(int(v) for v in L) for L in layers]
    n = len(layers)
    if n < 1 or any(len(L) != 8 for L in layers):
        raise ValueError("conv_pack_plan: layers is a non-empty list of (cout, cin, ks, stride, H, W, dgrad_form, src_off)")
    for L in layers:
        _stride_ok(L[2], L[3])
    cols = [(C.c_int32 * n)(*[L[j] for L in layers]) for j in range(7)]
    src = (C.c_int64 * n)(*[L[7] for L in layers])
    dst, cnt, total = (C.c_int64 * n)(), (C.c_int64 * n)(), C.c_int64(0)
    dev = torch.device(device)
    table = torch.zeros(_lib.PACK_TABLE_HEAD + n * _lib.PACK_TABLE_REC, dtype=torch.int64, device=dev)
    _call("obb_conv_pack_plan", ctx(dev), n, *cols, src, int(src_elems), dst, cnt, C.byref(total), _p(table), table.numel(), _stream())
    return PackTable(table, layers, list(dst), list(cnt), total.value, int(src_elems))


def conv_pack_multi_bf16(flat, plan, out=None):
    """Every layer of `plan` (a `PackTable`) packed from the flat fp32 weight buffer `flat` into ONE bf16 buffer of plan.total elements (`out`, or
    a new one) by ONE kernel launch: segment i = out[dst_off[i] : dst_off[i] + n_elems[i]] holds the bits `conv_pack_bf16` gives for layer i; the
    padding between segments is not written.  No host read, copy or synchronisation: it can sit inside a captured graph."""
    ff = _chk(flat, torch.float32, "flat")
    if ff.numel() != plan.src_elems:
        raise ValueError(f"conv_pack_multi_bf16: the plan was made for a flat buffer of {plan.src_elems} elements, got {ff.numel()}")
    out = torch.empty(plan.total, dtype=torch.bfloat16, device=ff.device) if out is None else _chk(out, torch.bfloat16, "out")
    if out.numel() != plan.total or out.device != ff.device or plan.table.device != ff.device:
        raise ValueError(f"conv_pack_multi_bf16: out holds {out.numel()} elements, the plan's total is {plan.total}: a plan for other layers or another map size?")
    _O.conv_pack_multi(ff, plan.table, plan.nrec, out)
    return out


def _check_packed(pk, fn, cout, cin, ks, H, W, stride=1, dgrad_form=False):
    """plan_conv picks the packed layout from the map size (13-multiple maps: single-stage WRES, CK = cin; others CK = 16): a blob packed for
    another H x W would be read in the wrong layout.  Its length tells the layouts apart."""
    n = _packed_elems(pk.device, cout, cin, ks, H, W, stride, dgrad_form)
    if pk.numel() != n:
        raise ValueError(f"{fn}: packed weights hold {pk.numel()} elements, {n} expected for {cin} -> {cout}, k {ks}, stride {stride} at {H} x {W}: "
                         "packed for another map size or layer?")


def conv_fwd_bf16(x, packed, bias, cout, ks, stride=1):
    """y = conv(x) + bias (`same` padding, no activation): x bf16 [B,H,W,cin] NHWC, packed = conv_pack_bf16 of the [cout,cin,ks,ks]
    weights for this H x W and stride, bias fp32 [cout] or None -> bf16 [B,Ho,Wo,cout] (stride 2, k 3: Ho = (H + 1) // 2)."""
    _stride_ok(ks, stride)
    xx = _chk(x, torch.bfloat16, "x")
    B, H, W, cin = xx.shape
    b = _chk(bias, torch.float32, "bias") if bias is not None else None
    pk = _chk(packed, torch.bfloat16, "packed")
    _check_packed(pk, "conv_fwd_bf16", int(cout), cin, ks, H, W, stride)
    if stride == 2:
        y = torch.empty((B, (H + 1) // 2, (W + 1) // 2, cout), dtype=torch.bfloat16, device=xx.device)
        _call("obb_conv_fwd_s2_bf16", ctx(xx.device), _p(xx), _p(pk), _p(b), B, H, W, cin, int(cout), _p(y), _stream())
        return y
    y = torch.empty((B, H, W, cout), dtype=torch.bfloat16, device=xx.device)
    _call("obb_conv_fwd_bf16", ctx(xx.device), _p(xx), _p(pk), _p(b), B, H, W, cin, int(cout), int(ks), _p(y), _stream())
    return y


def conv_dgrad_s2_bf16(dy, packed_dgrad, cin, H, W):
    """Input gradient of the stride-2 3x3 conv: dy bf16 [B,Ho,Wo,cout] -> dx bf16 [B,H,W,cin] (H, W: the forward's input size, Ho = (H + 1) // 2),
    packed_dgrad = conv_pack_bf16(w, H, W, dgrad_form=True).  Zero insertion + the stride-1 forward kernel: 4x the useful MACs."""
    d = _chk(dy, torch.bfloat16, "dy")
    B, Ho, Wo, cout = d.shape
    if (Ho, Wo) != ((H + 1) // 2, (W + 1) // 2):
        raise ValueError(f"conv_dgrad_s2_bf16: dy {tuple(d.shape)} is not the stride-2 output of {H} x {W}")
    pk = _chk(packed_dgrad, torch.bfloat16, "packed_dgrad")
    _check_packed(pk, "conv_dgrad_s2_bf16", cout, int(cin), 3, H, W, dgrad_form=True)
    dx = torch.empty((B, H, W, cin), dtype=torch.bfloat16, device=d.device)
    _call("obb_conv_dgrad_s2_bf16", ctx(d.device), _p(d), _p(pk), B, int(H), int(W), int(cin), cout, _p(dx),
          _stream())
    return dx


def _bn_fwd_body(fn, op, z, gamma, beta, running_mean, running_var, eps, momentum, *act):
    """The body of bn_silu_fwd_bf16 / bn_fwd_bf16 (`fn`: the public name; `op`: its registered op, the second one with `act` as last argument)."""
    zz = _chk(z, torch.bfloat16, "z")
    Cn = zz.shape[-1]
    vecs = [_chk(t, torch.float32, nm) for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var"))]
    if any(t.numel() != Cn for t in vecs):
        raise ValueError(f"{fn}: per-channel vectors must have C entries")
    a = torch.empty_like(zz)
    mean = torch.empty(Cn, dtype=torch.float32, device=zz.device)
    invstd = torch.empty_like(mean)
    op(zz, vecs[0], vecs[1], float(eps), float(momentum), vecs[2], vecs[3], mean, invstd, a, *act)
    return a, mean, invstd


def bn_silu_fwd_bf16(z, gamma, beta, running_mean, running_var, eps=1e-3, momentum=0.03):
    """Training-mode BatchNorm2d + SiLU over the rows of z bf16 [..., C] (NHWC): -> (a bf16 like z, batch mean fp32 [C], invstd fp32 [C]);
    running_mean / running_var (fp32 [C]) are updated in place with `momentum`, the running variance unbiased (torch's rule)."""
    return _bn_fwd_body("bn_silu_fwd_bf16", _O.bn_silu_fwd, z, gamma, beta, running_mean, running_var, eps, momentum)


def bn_fwd_bf16(z, gamma, beta, running_mean, running_var, eps=1e-3, momentum=0.03, act=True):
    """bn_silu_fwd_bf16 with the activation as an argument: act=True is that function (bit-identical), act=False the training-mode BatchNorm2d
    alone (Conv(act=False)) -> (a bf16 like z, batch mean fp32 [C], invstd fp32 [C])."""
    return _bn_fwd_body("bn_fwd_bf16", _O.bn_fwd, z, gamma, beta, running_mean, running_var, eps, momentum, bool(act))


def _bn_bwd_body(fn, op, z, da, gamma, beta, mean, invstd, dgamma, dbeta, *act):
    """The body of bn_silu_bwd_bf16 / bn_bwd_bf16, as _bn_fwd_body."""
    zz, d = _chk(z, torch.bfloat16, "z"), _chk(da, torch.bfloat16, "da")
    if d.shape != zz.shape:
        raise ValueError(f"{fn}: da must have the shape of z")
    Cn = zz.shape[-1]
    vecs = [_chk(t, torch.float32, nm) for t, nm in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (invstd, "invstd"))]
    dg = torch.empty(Cn, dtype=torch.float32, device=zz.device) if dgamma is None else _chk(dgamma, torch.float32, "dgamma")
    db = torch.empty(Cn, dtype=torch.float32, device=zz.device) if dbeta is None else _chk(dbeta, torch.float32, "dbeta")
    if any(t.numel() != Cn for t in vecs + [dg, db]):
        raise ValueError(f"{fn}: per-channel vectors must have C entries")
    dz = torch.empty_like(zz)
    op(zz, d, *vecs, dg, db, dz, *act)
    return dz, dg, db


def bn_silu_bwd_bf16(z, da, gamma, beta, mean, invstd, dgamma=None, dbeta=None):
    """Backward of bn_silu_fwd_bf16 (batch statistics): z, da bf16 [..., C] -> (dz bf16 like z, dgamma fp32 [C], dbeta fp32 [C]); dgamma / dbeta
    go into the given tensors (e.g. views of an optimiser group's gradient buffer) when passed."""
    return _bn_bwd_body("bn_silu_bwd_bf16", _O.bn_silu_bwd, z, da, gamma, beta, mean, invstd, dgamma, dbeta)


def bn_bwd_bf16(z, da, gamma, beta, mean, invstd, dgamma=None, dbeta=None, act=True):
    """Backward of bn_fwd_bf16 with the same `act` -> (dz bf16 like z, dgamma fp32 [C], dbeta fp32 [C]); dgamma / dbeta go into the given tensors
    when passed."""
    return _bn_bwd_body("bn_bwd_bf16", _O.bn_bwd, z, da, gamma, beta, mean, invstd, dgamma, dbeta, bool(act))


def _dw_weights(w, Cn, fn):
    ww = _chk(w, torch.float32, "w")
    if tuple(ww.shape) != (Cn, 1, 3, 3):
        raise ValueError(f"{fn}: w must be the depthwise 3x3 weights [C,1,3,3] = [{Cn},1,3,3], got {tuple(ww.shape)}")
    return ww


def dwconv3_fwd_bf16(x, w):
    """Depthwise 3x3 convolution (stride 1, pad 1, groups = C, no bias, no activation): x bf16 [B,H,W,C] NHWC, w fp32 MASTER weights [C,1,3,3]
    (rounded to bf16 as the kernel loads them: no pack step) -> z bf16 [B,H,W,C]; fp32 sums, taps in (ky, kx) order, one bf16 rounding."""
    xx = _chk(x, torch.bfloat16, "x")
    if xx.dim() != 4:
        raise ValueError("dwconv3_fwd_bf16: x must be [B,H,W,C]")
    ww = _dw_weights(w, xx.shape[-1], "dwconv3_fwd_bf16")
    z = torch.empty_like(xx)
    _O.dwconv3_fwd(xx, ww, z)
    return z


def dwconv3_bwd_bf16(x, dz, w, dw_out=None, need_dx=True):
    """Fused backward of dwconv3_fwd_bf16, both gradients from one pass over x and dz (bf16 [B,H,W,C]) -> (dx bf16 [B,H,W,C] or None when
    need_dx is False, dw fp32 [C,1,3,3]); dw goes into `dw_out` when given (e.g. a view of an optimiser group's gradient buffer).
    Deterministic (no atomics)."""
    xx, d = _chk(x, torch.bfloat16, "x"), _chk(dz, torch.bfloat16, "dz")
    if xx.dim() != 4 or d.shape != xx.shape:
        raise ValueError("dwconv3_bwd_bf16: x and dz must both be [B,H,W,C]")
    Cn = xx.shape[-1]
    ww = _dw_weights(w, Cn, "dwconv3_bwd_bf16")
    dw = torch.empty((Cn, 1, 3, 3), dtype=torch.float32, device=xx.device) if dw_out is None else _chk(dw_out, torch.float32, "dw_out")
    if tuple(dw.shape) != (Cn, 1, 3, 3):
        raise ValueError("dwconv3_bwd_bf16: dw_out must be [C,1,3,3]")
    dx = torch.empty_like(xx) if need_dx else None
    _O.dwconv3_bwd(xx, d, ww, dx, dw)
    return dx, dw


def dwconv3_bwd_geometry(B, H, W, C):
    """Host helper -> (rows per stripe, pixels per lane run, number of slabs, L): the split obb_dwconv3_bwd_bf16 uses at this shape; L is the
    longest chain of fp32 additions one dw element passes through."""
    out = (_ct.c_int32 * 4)()
    _lib.check(_lib.lib().obb_dwconv3_bwd_geometry(int(B), int(H), int(W), int(C), out))
    return tuple(int(v) for v in out)


def _head_weights(w, cin, fn):
    ww = _chk(w, torch.float32, "w")
    if ww.dim() == 4 and tuple(ww.shape[2:]) == (1, 1):
        ww = ww.view(ww.shape[0], ww.shape[1])
    if ww.dim() != 2 or ww.shape[1] != cin or not 1 <= ww.shape[0] <= 64:
        raise ValueError(f"{fn}: w must be the 1x1 weights [cout,cin(,1,1)] with cin = {cin}, 1 <= cout <= 64, got {tuple(w.shape)}")
    if cin % 8 or not 8 <= cin <= 512:
        raise ValueError(f"{fn}: cin = {cin} must be a multiple of 8 in [8, 512]")
    return ww


def headconv_fwd_bf16(x, w, bias=None):
    """Narrow-output 1x1 conv with bias (the head's plain Conv2d outputs: nc class logits, 1 angle logit): x bf16 [..., cin] NHWC, w fp32 MASTER
    weights [cout,cin] or [cout,cin,1,1] (rounded to bf16 as the kernel loads them), bias fp32 [cout] or None -> y FP32 [..., cout], dense rows
    of cout floats (what the losses read); fp32 sums, c ascending, the bias last.  cin % 8 == 0 (8 .. 512), cout 1 .. 64."""
    xx = _chk(x, torch.bfloat16, "x")
    if xx.dim() < 2:
        raise ValueError("headconv_fwd_bf16: x must be [..., cin]")
    ww = _head_weights(w, xx.shape[-1], "headconv_fwd_bf16")
    cout = ww.shape[0]
    bb = None if bias is None else _chk(bias, torch.float32, "bias")
    if bb is not None and bb.numel() != cout:
        raise ValueError("headconv_fwd_bf16: bias must have cout entries")
    y = torch.empty(tuple(xx.shape[:-1]) + (cout,), dtype=torch.float32, device=xx.device)
    if xx.numel():
        _O.headconv_fwd(xx, ww, bb, y)
    return y


def headconv_bwd_bf16(x, dy, w, dw_out=None, db_out=None, need_dx=True):
    """Fused backward of headconv_fwd_bf16, everything from one pass over x (bf16 [..., cin]) and dy (FP32 [..., cout], rounded to bf16 as it is
    loaded) -> (dx bf16 like x or None when need_dx is False, dw fp32 like w, db fp32 [cout]); dw / db go into `dw_out` / `db_out` when given (e.g.
    views of an optimiser group's gradient buffer).  Deterministic (no atomics)."""
    xx, d = _chk(x, torch.bfloat16, "x"), _chk(dy, torch.float32, "dy")
    if xx.dim() < 2 or d.shape[:-1] != xx.shape[:-1]:
        raise ValueError("headconv_bwd_bf16: x [..., cin] and dy [..., cout] must agree in every dimension but the last")
    ww = _head_weights(w, xx.shape[-1], "headconv_bwd_bf16")
    cout, cin = ww.shape
    if d.shape[-1] != cout:
        raise ValueError(f"headconv_bwd_bf16: dy has {d.shape[-1]} channels, w {cout} outputs")
    dw = torch.empty_like(w) if dw_out is None else _chk(dw_out, torch.float32, "dw_out")
    db = torch.empty(cout, dtype=torch.float32, device=xx.device) if db_out is None else _chk(db_out, torch.float32, "db_out")
    if dw.numel() != cout * cin or db.numel() != cout:
        raise ValueError("headconv_bwd_bf16: dw_out must have the size of w, db_out cout entries")
    dx = torch.empty_like(xx) if need_dx else None
    if not xx.numel():
        raise ValueError("headconv_bwd_bf16: no pixels")
    _O.headconv_bwd(xx, d, ww, dx, dw, db)
    return dx, dw, db


def headconv_bwd_geometry(N, cin, cout):
    """Host helper -> (pixels per lane run, lane rows per workgroup RP, number of slabs nbx, L): the split obb_headconv_bwd_bf16 uses at this shape
    (lane row r of workgroup bx walks pixels bx RP + r + t nbx RP); L is the longest chain of fp32 additions one dw / db element passes through."""
    out = (_ct.c_int32 * 4)()
    _lib.check(_lib.lib().obb_headconv_bwd_geometry(int(N), int(cin), int(cout), out))
    return tuple(int(v) for v in out)


def _stem_args(x, w_shape, fn):
    xx = _chk(x, torch.uint8, "x")
    if xx.dim() != 4 or xx.shape[-1] not in (3, 4):
        raise ValueError(f"{fn}: x must be the uint8 tile [B,H,W,3 or 4], got {tuple(xx.shape)}")
    cin = xx.shape[-1]
    if len(w_shape) != 4 or tuple(w_shape[1:]) != (cin, 3, 3) or w_shape[0] % 8 or not 8 <= w_shape[0] <= 64:
        raise ValueError(f"{fn}: w must be [cout,{cin},3,3] with cout a multiple of 8 in [8, 64], got {tuple(w_shape)}")
    return xx


def stemconv_fwd_u8(x, w):
    """The stem's conv (3x3, stride 2, pad 1, no bias) straight from the uint8 tile: x uint8 [B,H,W,cin] (cin 3 or 4, channel order as stored), w
    fp32 MASTER weights [cout,cin,3,3] -> z bf16 [B,(H+1)//2,(W+1)//2,cout]; the operand is bf16(v / 255), fp32 sums, one bf16 rounding."""
    ww = _chk(w, torch.float32, "w")
    xx = _stem_args(x, ww.shape, "stemconv_fwd_u8")
    B, H, W, _ = xx.shape
    z = torch.empty((B, (H + 1) // 2, (W + 1) // 2, ww.shape[0]), dtype=torch.bfloat16, device=xx.device)
    if z.numel():
        _O.stemconv_fwd(xx, ww, z)
    return z


def stemconv_wgrad_u8(x, dz, out=None):
    """dW of stemconv_fwd_u8: x uint8 [B,H,W,cin], dz bf16 [B,(H+1)//2,(W+1)//2,cout] -> dw fp32 [cout,cin,3,3] (into `out` when given).  There is
    no input gradient: the input is the image.  Deterministic (no atomics)."""
    d = _chk(dz, torch.bfloat16, "dz")
    if d.dim() != 4:
        raise ValueError("stemconv_wgrad_u8: dz must be [B,Ho,Wo,cout]")
    cout = d.shape[-1]
    xx = _stem_args(x, (cout, x.shape[-1] if x.dim() == 4 else 0, 3, 3), "stemconv_wgrad_u8")
    B, H, W, cin = xx.shape
    if tuple(d.shape[:3]) != (B, (H + 1) // 2, (W + 1) // 2) or not d.numel():
        raise ValueError(f"stemconv_wgrad_u8: dz {tuple(d.shape)} is not the stride-2 output of {tuple(xx.shape)}")
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=xx.device) if out is None else _chk(out, torch.float32, "out")
    if tuple(dw.shape) != (cout, cin, 3, 3):
        raise ValueError(f"stemconv_wgrad_u8: out must be [{cout},{cin},3,3]")
    _O.stemconv_wgrad(xx, d, dw)
    return dw


def stemconv_wgrad_geometry(B, H, W, cin, cout):
    """Host helper -> (output pixels per lane run, lane rows per workgroup RP, number of slabs nbx, L): the split obb_stemconv_wgrad_u8 uses at this
    shape (lane row r of workgroup bx walks output pixels bx RP + r + t nbx RP); L as for headconv_bwd_geometry."""
    out = (_ct.c_int32 * 4)()
    _lib.check(_lib.lib().obb_stemconv_wgrad_geometry(int(B), int(H), int(W), int(cin), int(cout), out))
    return tuple(int(v) for v in out)


def sppf_pools_fwd_bf16(x):
    """The three chained 5x5 max pools of SPPF (stride 1, pad 2): x bf16 [B,H,W,C] -> cat bf16 [B,H,W,4C] = [x, y1, y2, y3], bit-equal to
    F.max_pool2d on the same values.  H, W <= 32 (the map of a workgroup's channels is resident in LDS)."""
    xx = _chk(x, torch.bfloat16, "x")
    if xx.dim() != 4:
        raise ValueError("sppf_pools_fwd_bf16: x must be [B,H,W,C]")
    B, H, W, Cn = xx.shape
    cat = torch.empty((B, H, W, 4 * Cn), dtype=torch.bfloat16, device=xx.device)
    _O.sppf_pools_fwd(xx, cat)
    return cat


def sppf_pools_bwd_bf16(cat, dcat):
    """Backward of sppf_pools_fwd_bf16 from cat and dcat (bf16 [B,H,W,4C]) alone -> dx bf16 [B,H,W,C]; the argmax is recomputed (first maximum
    in row-major scan of the window, torch's rule), fp32 sums, one bf16 rounding."""
    c, d = _chk(cat, torch.bfloat16, "cat"), _chk(dcat, torch.bfloat16, "dcat")
    if c.dim() != 4 or c.shape != d.shape or c.shape[-1] % 4:
        raise ValueError("sppf_pools_bwd_bf16: cat and dcat must both be [B,H,W,4C]")
    B, H, W, C4 = c.shape
    dx = torch.empty((B, H, W, C4 // 4), dtype=torch.bfloat16, device=c.device)
    _O.sppf_pools_bwd(c, d, dx)
    return dx


def upcat_fwd_bf16(a, b, up=1):
    """cat(nearest_upsample_up(a), b) along C, a first (Ultralytics' Concat([-1, skip])): a bf16 [B,H,W,Ca], b bf16 [B,up H,up W,Cb] ->
    bf16 [B,up H,up W,Ca+Cb]; up = 1 is the plain concat."""
    aa, bb = _chk(a, torch.bfloat16, "a"), _chk(b, torch.bfloat16, "b")
    if aa.dim() != 4 or bb.dim() != 4 or up < 1 or tuple(bb.shape[:3]) != (aa.shape[0], aa.shape[1] * up, aa.shape[2] * up):
        raise ValueError(f"upcat_fwd_bf16: a {tuple(aa.shape)} upsampled by {up} does not match b {tuple(bb.shape)}")
    out = torch.empty((*bb.shape[:3], aa.shape[3] + bb.shape[3]), dtype=torch.bfloat16, device=aa.device)
    _O.upcat_fwd(aa, bb, int(up), out)
    return out


def upcat_bwd_bf16(dout, Ca, up=1, da=None, db=None, need_da=True, need_db=True):
    """Backward of upcat_fwd_bf16: dout bf16 [B,up H,up W,Ca+Cb] -> (da bf16 [B,H,W,Ca], db bf16 [B,up H,up W,Cb]).  A GIVEN da / db is
    accumulated into (read, fp32 add, one rounding: the gradient sum of a tensor with two consumers); None allocates and overwrites.
    need_da / need_db = False skips that half (None is returned for it)."""
    d = _chk(dout, torch.bfloat16, "dout")
    if d.dim() != 4 or up < 1 or d.shape[1] % up or d.shape[2] % up:
        raise ValueError(f"upcat_bwd_bf16: dout {tuple(d.shape)} is not a map upsampled by {up}")
    B, uH, uW, Co = d.shape
    H, W, Cb = uH // up, uW // up, Co - int(Ca)
    acc_a, acc_b = need_da and da is not None, need_db and db is not None
    if need_da:
        da = torch.empty((B, H, W, int(Ca)), dtype=torch.bfloat16, device=d.device) if da is None else _chk(da, torch.bfloat16, "da")
        if tuple(da.shape) != (B, H, W, int(Ca)):
            raise ValueError("upcat_bwd_bf16: da must be [B,H,W,Ca]")
    else:
        da = None
    if need_db:
        db = torch.empty((B, uH, uW, Cb), dtype=torch.bfloat16, device=d.device) if db is None else _chk(db, torch.bfloat16, "db")
        if tuple(db.shape) != (B, uH, uW, Cb):
            raise ValueError("upcat_bwd_bf16: db must be [B,up H,up W,Cb]")
    else:
        db = None
    _O.upcat_bwd(d, H, W, int(Ca), int(up), da, db, acc_a, acc_b)
    return da, db


def _attn_tokens(t, nh, per_head, fn, name):
    """t bf16 [B, ..., nh * per_head] with at least one token axis -> (checked tensor, B, N)"""
    tt = _chk(t, torch.bfloat16, name)
    if int(nh) < 1 or tt.dim() < 3 or tt.shape[-1] != int(nh) * per_head:
        raise ValueError(f"{fn}: {name} must be [B, ..., nh * {per_head}] = [B, ..., {int(nh) * per_head}] for nh = {nh}, got {tuple(tt.shape)}")
    return tt, tt.shape[0], tt.numel() // (tt.shape[0] * tt.shape[-1])


def attn_fwd_bf16(qkv, nh):
    """Softmax attention core with key_dim 32, head_dim 64: qkv bf16 [B, N, nh * 128] (or [B, H, W, nh * 128], N = H W), per token
    [q: nh * 32 | k: nh * 32 | v: nh * 64] -> (out bf16 [B, ..., nh * 64], lse fp32 [B, nh, N]); 1 <= N <= 192.  lse is all the backward needs."""
    qq, B, N = _attn_tokens(qkv, nh, 128, "attn_fwd_bf16", "qkv")
    out = torch.empty((*qq.shape[:-1], int(nh) * 64), dtype=torch.bfloat16, device=qq.device)
    lse = torch.empty((B, int(nh), N), dtype=torch.float32, device=qq.device)
    _O.attn_fwd(qq, int(nh), out, lse)
    return out, lse


def attn_bwd_bf16(qkv, out, lse, dout, nh, dv_add=None):
    """Backward of attn_fwd_bf16 -> dqkv bf16 like qkv, every element written.  dv_add (bf16 like out) is added to dV in fp32 before its one
    rounding: the gradient of v's other consumer.  Deterministic (no atomics)."""
    qq, B, N = _attn_tokens(qkv, nh, 128, "attn_bwd_bf16", "qkv")
    oo, _, _ = _attn_tokens(out, nh, 64, "attn_bwd_bf16", "out")
    dd, _, _ = _attn_tokens(dout, nh, 64, "attn_bwd_bf16", "dout")
    ll = _chk(lse, torch.float32, "lse")
    if oo.shape[:-1] != qq.shape[:-1] or dd.shape != oo.shape or tuple(ll.shape) != (B, int(nh), N):
        raise ValueError(f"attn_bwd_bf16: out {tuple(oo.shape)}, dout {tuple(dd.shape)}, lse {tuple(ll.shape)} do not belong to qkv {tuple(qq.shape)}")
    if dv_add is not None:
        dv_add, _, _ = _attn_tokens(dv_add, nh, 64, "attn_bwd_bf16", "dv_add")
        if dv_add.shape != oo.shape:
            raise ValueError("attn_bwd_bf16: dv_add must have the shape of out")
    dqkv = torch.empty_like(qq)
    _O.attn_bwd(qq, oo, ll, dd, dv_add, int(nh), dqkv)
    return dqkv


def add_bf16(a, b, out=None):
    """bf16(fp32(a) + fp32(b)) element-wise, numel % 8 == 0; `out` may be `a` (in place)."""
    aa, bb = _chk(a, torch.bfloat16, "a"), _chk(b, torch.bfloat16, "b")
    if aa.shape != bb.shape:
        raise ValueError(f"add_bf16: a {tuple(aa.shape)} and b {tuple(bb.shape)} differ in shape")
    out = torch.empty_like(aa) if out is None else _chk(out, torch.bfloat16, "out")
    if out.shape != aa.shape:
        raise ValueError("add_bf16: out must have the shape of a")
    _O.add_bf16(aa, bb, out)
    return out


def chanwin_bf16(src, s0, n, dst=None, d0=0, add=None, a0=0):
    """dst[..., d0:d0+n] = src[..., s0:s0+n] (+ add[..., a0:a0+n]: fp32 add, one rounding) over bf16 tensors that share their leading dims; the
    other channels of dst stay as they are.  dst None allocates a dense [..., n] tensor (then d0 must be 0).  Without add the values are copied as
    bits.  The chunk / split / cat of C3k2 and C2PSA and the gradient sums at their concat members; offsets and widths in multiples of 8."""
    ss = _chk(src, torch.bfloat16, "src")
    if ss.dim() < 2:
        raise ValueError("chanwin_bf16: src must be [..., C]")
    if add is not None:
        add = _chk(add, torch.bfloat16, "add")
        if add.shape[:-1] != ss.shape[:-1]:
            raise ValueError(f"chanwin_bf16: add {tuple(add.shape)} and src {tuple(ss.shape)} differ in their leading dims")
    if dst is None:
        if d0 != 0 or int(n) < 1:
            raise ValueError(f"chanwin_bf16: without dst the result is dense: d0 = {d0} must be 0 and n = {n} positive")
        dst = torch.empty((*ss.shape[:-1], int(n)), dtype=torch.bfloat16, device=ss.device)
    else:
        dst = _chk(dst, torch.bfloat16, "dst")
        if dst.shape[:-1] != ss.shape[:-1]:
            raise ValueError(f"chanwin_bf16: dst {tuple(dst.shape)} and src {tuple(ss.shape)} differ in their leading dims")
    _O.chanwin(ss, int(s0), add, int(a0), int(n), dst, int(d0))
    return dst


def silu_bf16(z):
    zz = _chk(z, torch.bfloat16, "z")
    a = torch.empty_like(zz)
    _call("obb_silu_bf16", ctx(zz.device), _p(zz), _p(a), zz.numel(), _stream())
    return a


def silu_bwd_bf16(z, da):
    zz, d = _chk(z, torch.bfloat16, "z"), _chk(da, torch.bfloat16, "da")
    dz = torch.empty_like(zz)
    _call("obb_silu_bwd_bf16", ctx(zz.device), _p(zz), _p(d), _p(dz), zz.numel(), _stream())
    return dz


def bias_grad_bf16(dy, out=None):
    d = _chk(dy, torch.bfloat16, "dy")
    cout = d.shape[-1]
    db = _chk(out, torch.float32, "out") if out is not None else torch.empty(cout, dtype=torch.float32, device=d.device)
    if db.numel() != cout:
        raise ValueError(f"bias_grad_bf16: out has {db.numel()} entries, dy has {cout} channels")
    _call("obb_bias_grad_bf16", ctx(d.device), _p(d), d.numel() // cout, cout, _p(db), _stream())
    return db


def tile_survivors(det, count, lb, tile_ids, rects, margin, iou_thr, strike_cls=1):
    """det float32[B, max_det, 7] + count int32[B] (decode_nms) -> (records int32[B * max_det, 12] (capacity), tile_off int32[B + 1],
    n_records int32[1]), all on the device: result construction, per-detection body (border filter `margin`), per-tile merge at `iou_thr`
    and compaction into exchange records in tile order, with no host-visible count in between."""
    d = _chk(det, torch.float32, "det")
    c = _chk(count, torch.int32, "count")
    ti = _chk(tile_ids, torch.int32, "tile_ids")
    r = _chk(rects, torch.int32, "rects").reshape(-1, 4)
    if lb is not None:
        lb = _chk(lb, torch.float32, "lb").reshape(-1, 3)
    B, md = d.shape[0], d.shape[1]
    rec = torch.empty((B * md, 12), dtype=torch.int32, device=d.device)
    off = torch.empty(B + 1, dtype=torch.int32, device=d.device)
    n = torch.empty(1, dtype=torch.int32, device=d.device)
    _O.tile_survivors(d, c, lb, ti, r, int(margin), int(strike_cls), float(iou_thr), rec, off, n)
    return rec, off, n


def select_kept(order, keep, boxes, cls, conf, angle):
    """rows order[i] of the sorted positions i with keep[i], in that order -> (boxes, cls, conf, angle) of capacity n and n_out int32[1] (device)"""
    n = order.shape[0]
    ob = torch.empty((n, 8), dtype=torch.float64, device=order.device)
    oc = torch.empty(n, dtype=torch.int32, device=order.device)
    of = torch.empty(n, dtype=torch.float64, device=order.device)
    oa = torch.empty(n, dtype=torch.float64, device=order.device)
    cnt = torch.empty(1, dtype=torch.int32, device=order.device)
    _O.select_kept(_chk(order, torch.int32, "order"), _chk(keep, torch.uint8, "keep"), _chk(boxes, torch.float64, "boxes"), _chk(cls, torch.int32, "cls"),
                   _chk(conf, torch.float64, "conf"), _chk(angle, torch.float64, "angle"), ob, oc, of, oa, cnt)
    return ob, oc, of, oa, cnt


def records_to_dets(records, n, rects, strike_cls=1):
    """the first n rows of packed records int32[*, 12] -> (global boxes float64[n, 8], cls int32[n], conf float64[n], angle float64[n])"""
    rec = _chk(records, torch.int32, "records")
    r = _chk(rects, torch.int32, "rects").reshape(-1, 4)
    n = int(n)
    gb = torch.empty((n, 8), dtype=torch.float64, device=rec.device)
    c = torch.empty(n, dtype=torch.int32, device=rec.device)
    f = torch.empty(n, dtype=torch.float64, device=rec.device)
    a = torch.empty(n, dtype=torch.float64, device=rec.device)
    if n:
        _O.records_to_dets(rec, n, r, int(strike_cls), gb, c, f, a)
    return gb, c, f, a


def gather_compact(recv):
    """recv int32[world, capacity + 1, 12] (all_gather of fixed-capacity record blocks, count in [w, 0, 0]) -> (rows int32[world * capacity, 12]
    dense in rank order, counts int32[world + 1]: the counts as sent, then the number of rows written)"""
    r = _chk(recv, torch.int32, "recv")
    world, cap = r.shape[0], r.shape[1] - 1
    out = torch.empty((world * cap, 12), dtype=torch.int32, device=r.device)
    counts = torch.empty(world + 1, dtype=torch.int32, device=r.device)
    _O.gather_compact(r, out, counts)
    return out, counts


PRECISIONS = {"f16": 16, "fp16": 16, "bf16": 1016, "f32": 32, "fp32": 32}
# engine switches of obb_set_option (each restores the separate launches of one fused form; used by the A/B parity tests)
MODEL_OPTIONS = ("fuse", "tail", "tail16", "bneck", "bneck_cv2", "c3kimg", "dwpw", "upfold", "stem", "front", "pair", "hmerge", "sppf_fuse", "attn_mfma", "xtile", "nitile", "nc2", "blk32", "c3k2f", "pw32", "upacc", "graph")


def select_model(slot, device=None):
    """Several models can live in one context (dual-scale); choose which one load/forward/decode address."""
    _call("obb_set_option", ctx(device), b"model_slot", int(slot))


def get_option(key, device=None):
    """What obb_set_option last set for `key` ("model_slot": the active slot; "precision": 16 / 1016 / 32; a switch of MODEL_OPTIONS: 0 / 1)."""
    v = C.c_int64(0)
    _call("obb_get_option", ctx(device), key.encode(), C.byref(v))
    return v.value


@contextlib.contextmanager
def engine_state(device=None):
    """Inside: load, select and run models freely; on exit the context's active model slot and every option are as they were on entry (a
    component with a model of its own, like train.Validator, next to the application's models)."""
    keys = ("precision",) + MODEL_OPTIONS[1:]  # what `select_model` / `model_load` set; the other options nobody inside touches
    c = ctx(device)
    slot, saved = get_option("model_slot", device), {k: get_option(k, device) for k in keys}
    try:
        yield
    finally:
        for k, v in saved.items():
            _call("obb_set_option", c, k.encode(), v)
        _call("obb_set_option", c, b"model_slot", slot)


def model_load(blob, device=None, precision="f16", fuse=False, tail=True, **options):
    """blob: bytes of an "OBBW" weight blob (host), loaded into the active model slot.  precision: "f16" / "bf16" = 16-bit storage with
    fp32 accumulation, "f32" = fp32 arithmetic end to end (what the reference computes; one kernel per layer).
    tail=False keeps the final 1x1 conv of each head branch a separate launch and turns every other intermediate-swallowing fusion off
    (every layer observable).  Further keyword switches (MODEL_OPTIONS, all default on except `fuse`) disable single fused forms:
    tail16, bneck, bneck_cv2, c3kimg, dwpw, upfold, stem, front, pair, hmerge, sppf_fuse, attn_mfma, xtile, nitile, nc2, blk32, c3k2f, pw32, upacc."""
    c = ctx(device)
    _call("obb_set_option", c, b"precision", PRECISIONS[precision])
    _call("obb_set_option", c, b"fuse", 1 if fuse else 0)
    _call("obb_set_option", c, b"tail", 1 if tail else 0)
    for k in MODEL_OPTIONS[2:]:
        try:
            _call("obb_set_option", c, k.encode(), 1 if options.pop(k, True) else 0)
        except _lib.ObbHipError:
            if not os.environ.get("OBB_LIB"):  # (an older diagnostic build named by OBB_LIB may not know the newest switches: A/B timing only)
                raise
    if options:
        raise TypeError(f"model_load: unknown options {sorted(options)}")
    mv = memoryview(blob)
    buf = (C.c_char * mv.nbytes).from_buffer(mv) if not mv.readonly else (C.c_char * mv.nbytes).from_buffer_copy(mv)  # (the library copies it anyway)
    _call("obb_model_load", c, buf, mv.nbytes)


def model_unload(slot, device=None):
    """Frees the model of `slot` (weights, plans, activation slabs, captured graphs) after a device synchronisation."""
    _call("obb_model_unload", ctx(device), int(slot))


def model_info(h, w, device=None):
    c = ctx(device)
    nc, ch, a, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    _call("obb_model_info", c, h, w, C.byref(nc), C.byref(ch), C.byref(a), C.byref(n))
    return {"nc": nc.value, "ch": ch.value, "anchors": a.value, "nconv": n.value}


def forward(tiles, out=None, cmax=None):
    """tiles uint8 [B,h,w,ch] NHWC (BGR for 3-channel input, as the reference passes crops) -> raw head [B,A,NO] f32.
    `out`: optional preallocated head tensor (stable input/output addresses let the library replay its captured hipGraph).
    `cmax`: optional float32 [B,A] that receives the largest class logit of every anchor (the dense candidate gate of
    decode_nms(..., cmax=...): obb_forward_gate)."""
    t = _chk(tiles, torch.uint8, "tiles")
    B, h, w, ch = t.shape
    info = model_info(h, w, t.device)
    if ch != info["ch"]:
        raise ValueError(f"forward: model expects {info['ch']} input channels, got {ch}")
    no = 64 + info["nc"] + 1
    shape = (B, info["anchors"], (no + 3) // 4 * 4)
    if out is not None:
        if tuple(out.shape) != shape:
            raise ValueError(f"forward: out must have shape {shape}")
        head = _chk(out, torch.float32, "out")
    else:
        head = torch.zeros(shape, dtype=torch.float32, device=t.device)
    if cmax is not None:
        cm = _chk(cmax, torch.float32, "cmax")
        if tuple(cm.shape) != shape[:2]:
            raise ValueError(f"forward: cmax must have shape {shape[:2]}")
        if B:
            _O.forward_gate(t, head, cm)
    elif B:
        _O.forward(t, head)
    return head  # rows padded to a multiple of 4 floats; [..., :64+nc+1] are the logits


def _padded_head(hd):
    """accept unpadded [B,A,64+nc+1] heads (e.g. from the oracle) by padding rows to the device layout"""
    no = hd.shape[-1]
    if no % 4 == 0:
        return hd
    out = torch.zeros(hd.shape[:-1] + ((no + 3) // 4 * 4,), dtype=hd.dtype, device=hd.device)
    out[..., :no] = hd
    return out


def debug_plan(h, w, device=None):
    """-> list of text lines, one per kernel launch of the lowered forward (layer, tiling, grid, LDS, MACs)"""
    c = ctx(device)
    need = C.c_int64(0)
    _call("obb_debug_plan", c, h, w, None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value)
    _call("obb_debug_plan", c, h, w, buf, need.value, C.byref(need))
    return buf.value.decode().strip().split("\n")


def debug_activation(name, B, h, w, device=None):
    c = ctx(device)
    n = C.c_int64(0)
    shp = (C.c_int32 * 3)()
    _call("obb_debug_activation", c, h, w, B, name.encode(), None, 0, C.byref(n), shp, _stream())
    out = torch.empty((B, shp[0], shp[1], shp[2]), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    _O.debug_activation(name, B, h, w, out)
    return out


def decode(head, h, w):
    """raw head [B,A,64+nc+1] -> predictions [B,A,4+nc+1] (x,y,w,h, class scores, theta); anchor-major."""
    hd = _padded_head(_chk(head, torch.float32, "head"))
    B, A, _ = hd.shape
    pred = torch.empty((B, A, 4 + model_info(h, w, hd.device)["nc"] + 1), dtype=torch.float32, device=hd.device)
    _O.decode(hd, h, w, pred)
    return pred


def decode_nms(head, h, w, conf=0.25, iou=0.7, max_det=300, full=False, zero=True, cmax=None):
    """-> (det [B,max_det,7] rows (x,y,w,h,conf,cls,theta) in score order, count int32[B]).  full=True runs the reference form (decode
    every anchor first) that the candidate-first default must reproduce bit for bit.  zero=False leaves the rows past count[b]
    uninitialised (no fill launch: what the device-side consumers, which only look at rows below the count, ask for)."""
    hd = _padded_head(_chk(head, torch.float32, "head"))
    B = hd.shape[0]
    det = (torch.zeros if zero or not B else torch.empty)((B, max_det, 7), dtype=torch.float32, device=hd.device)
    count = (torch.zeros if zero or not B else torch.empty)(B, dtype=torch.int32, device=hd.device)
    if B and cmax is not None and not full:
        cm = _chk(cmax, torch.float32, "cmax")
        if tuple(cm.shape) != tuple(hd.shape[:2]):
            raise ValueError("decode_nms: cmax must be [B, A] of the same head")
        _O.decode_nms_gate(hd, cm, h, w, float(conf), float(iou), int(max_det), det, count)
    elif B:
        (_O.decode_nms_full if full else _O.decode_nms)(hd, h, w, float(conf), float(iou), int(max_det), det, count)
    return det, count


def probiou_nms(boxes, scores, iou):
    b = _chk(boxes, torch.float32, "boxes").reshape(-1, 5)
    s = _chk(scores, torch.float32, "scores")
    n = b.shape[0]
    order = torch.empty(n, dtype=torch.int32, device=b.device)
    keep = torch.zeros(n, dtype=torch.uint8, device=b.device)
    _O.probiou_nms(b, s, float(iou), order, keep)
    return order, keep


def results(det, lb=None):
    """det [n,7] rows from decode_nms -> (xywhr [n,5] regularised + un-letterboxed, corners [n,8])"""
    d = _chk(det, torch.float32, "det").reshape(-1, 7)
    n = d.shape[0]
    if lb is not None:
        lb = _chk(lb, torch.float32, "lb").reshape(-1, 3)
    xywhr = torch.empty((n, 5), dtype=torch.float32, device=d.device)
    pts = torch.empty((n, 8), dtype=torch.float32, device=d.device)
    _O.results(d, lb, xywhr, pts)
    return xywhr, pts


def gather_tiles(image, rects, tile):
    """image uint8 [H,W,C] (device), rects int32 [n,4] (device, all tile x tile) -> uint8 [n,tile,tile,C]"""
    img = _chk(image, torch.uint8, "image")
    r = _chk(rects, torch.int32, "rects").reshape(-1, 4)
    H, W, Cc = img.shape
    out = torch.empty((r.shape[0], tile, tile, Cc), dtype=torch.uint8, device=img.device)
    _O.gather_tiles(img, r, int(tile), out)
    return out


def letterbox_shape(ch, cw, imgsz, stride=32):
    """Host arithmetic of LetterBox(auto=True): -> dict(out_h, out_w, gain, pad_x, pad_y)"""
    r = min(imgsz / ch, imgsz / cw)
    new_w, new_h = int(round(cw * r)), int(round(ch * r))
    dw, dh = ((imgsz - new_w) % stride) / 2, ((imgsz - new_h) % stride) / 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    out_h, out_w = new_h + top + bottom, new_w + left + right
    # un-letterbox parameters exactly as scale_boxes computes them from the two shapes
    gain = min(out_h / ch, out_w / cw)
    pad_x = round((out_w - cw * gain) / 2 - 0.1)
    pad_y = round((out_h - ch * gain) / 2 - 0.1)
    return {"out_h": out_h, "out_w": out_w, "gain": gain, "pad_x": pad_x, "pad_y": pad_y}


def letterbox(image, x, y, x2, y2, imgsz):
    img = _chk(image, torch.uint8, "image")
    H, W, Cc = img.shape
    p = letterbox_shape(y2 - y, x2 - x, imgsz)
    out = torch.empty((p["out_h"], p["out_w"], Cc), dtype=torch.uint8, device=img.device)
    _O.letterbox(img, int(x), int(y), int(x2), int(y2), int(imgsz), out)
    return out, p


def tile_labels(labels, rects, min_fraction=0.1):
    """Training-set tiler, label assignment (Train_OBB.py:87-112): labels float64 [n,8] pixel corners, rects int32 [T,4] square tiles ->
    (mask uint8 [T,n], out float64 [T,n,8] = shifted / clipped / normalised corners where mask is set, zeros elsewhere)."""
    lab = _chk(labels, torch.float64, "labels").reshape(-1, 8)
    r = _chk(rects, torch.int32, "rects").reshape(-1, 4)
    mask = torch.zeros((r.shape[0], lab.shape[0]), dtype=torch.uint8, device=lab.device)
    out = torch.zeros((r.shape[0], lab.shape[0], 8), dtype=torch.float64, device=lab.device)
    if lab.shape[0] and r.shape[0]:
        _O.tile_labels(lab, r, float(min_fraction), mask, out)
    return mask, out


def _aug_table(table, fn):
    t = _chk(table, torch.uint8, "table")
    if t.dim() != 2 or t.shape[1] != _lib.AUG_REC_BYTES:
        raise ValueError(f"{fn}: table must be uint8 [B, {_lib.AUG_REC_BYTES}] (augment.REC records), got {tuple(t.shape)}")
    return t


def aug_tiles(pool, table, bgr=True, swap_rb=False, out=None):
    """The augmentation's pixel kernel (obb_aug_tiles): pool uint8 [N,s,s,C] (C = 3 or 4), table uint8 [B,904] (augment.REC records, on the device) ->
    uint8 [B,s,s,C]: mosaic canvas, affine warp in warpAffine's fixed point, flips and HSV gains in one gather.  `out`: write into this buffer."""
    p = _chk(pool, torch.uint8, "pool")
    if p.dim() != 4:
        raise ValueError("aug_tiles: pool must be [N, s, s, C]")
    t = _aug_table(table, "aug_tiles")
    N, s, s2, Cc = p.shape
    if s != s2:
        raise ValueError("aug_tiles: pool tiles must be square")
    if out is None:
        out = torch.empty((t.shape[0], s, s, Cc), dtype=torch.uint8, device=p.device)
    elif _chk(out, torch.uint8, "out").shape != (t.shape[0], s, s, Cc):
        raise ValueError(f"aug_tiles: out must be {(t.shape[0], s, s, Cc)}, got {tuple(out.shape)}")
    _O.aug_tiles(p, t, bool(bgr), bool(swap_rb), out)
    return out


def aug_labels(pool_labels, pool_counts, table, s, n_cap, wh_thr=2.0, ar_thr=100.0, area_thr=0.01, out=None):
    """The augmentation's label kernel (obb_aug_labels): pool_labels float64 [N,Lmax,9] (class + 8 normalised corners), pool_counts int32 [N], the same
    table -> (gt_labels int32 [B,n_cap], gt_bboxes fp32 [B,n_cap,5], mask_gt bool [B,n_cap], count int32 [B]) as OBBCriterion reads them; count is the
    true number of survivors per tile, also past n_cap.  `out`: the four buffers to write into.  No host read."""
    pl = _chk(pool_labels, torch.float64, "pool_labels")
    pc = _chk(pool_counts, torch.int32, "pool_counts")
    t = _aug_table(table, "aug_labels")
    if pl.dim() != 3 or pl.shape[2] != 9 or pc.shape != (pl.shape[0],):
        raise ValueError("aug_labels: pool_labels must be [N, Lmax, 9] and pool_counts [N]")
    B, n_cap = t.shape[0], int(n_cap)
    if n_cap < 1:
        raise ValueError("aug_labels: n_cap must be at least 1")
    if out is None:
        out = (torch.empty((B, n_cap), dtype=torch.int32, device=pl.device), torch.empty((B, n_cap, 5), dtype=torch.float32, device=pl.device),
               torch.empty((B, n_cap), dtype=torch.bool, device=pl.device), torch.empty((B,), dtype=torch.int32, device=pl.device))
    gl, gb, mk, cnt = out
    _chk(gl, torch.int32, "gt_labels"); _chk(gb, torch.float32, "gt_bboxes"); _chk(mk, torch.bool, "mask_gt"); _chk(cnt, torch.int32, "count")
    if gl.shape != (B, n_cap) or gb.shape != (B, n_cap, 5) or mk.shape != (B, n_cap) or cnt.shape != (B,):
        raise ValueError("aug_labels: output buffers must be [B, n_cap], [B, n_cap, 5], [B, n_cap], [B]")
    _O.aug_labels(pl, pc, t, int(s), float(wh_thr), float(ar_thr), float(area_thr), gl, gb, mk, cnt)
    return gl, gb, mk, cnt


class FoldTable:
    """What `fold_blob_plan` returns: `table` (int64 device tensor: the head and records of csrc/foldblob.hip's k_fold_blob), `host` (its numpy
    copy), `nrec`, `out_elems` (fp32 elements of the blob's data section) and `need` (elements read up to in w_flat, g_flat, b_flat, buffers)."""

    def __init__(self, table, host, nrec, out_elems, need):
        self.table, self.host, self.nrec, self.out_elems, self.need = table, host, nrec, out_elems, need


def fold_blob_table(records):
    """The host table of `fold_blob_f32` (include/obbhip.h), numpy int64: records = [(kind, w_off, g_off, b_off, mean_off, var_off, cout, per)] in
    blob order, kind one of _lib.FOLD_BN / FOLD_PLAIN / FOLD_QKV, per = the weight elements per output channel; the destinations are dense: record
    i's cout * per weights, then its cout biases, behind record i - 1's."""
    import numpy as np
    recs = [tuple(int(v) for v in r) for r in records]
    if not recs or any(len(r) != 8 for r in recs):
        raise ValueError("fold_blob_table: records is a non-empty list of (kind, w_off, g_off, b_off, mean_off, var_off, cout, per)")
    H, R = _lib.FOLD_TABLE_HEAD, _lib.FOLD_TABLE_REC
    tab = np.zeros(H + len(recs) * R, np.int64)
    dst, wg, need = 0, 0, [0, 0, 0, 0]
    for i, (kind, w_off, g_off, b_off, m_off, v_off, cout, per) in enumerate(recs):
        if kind not in (_lib.FOLD_BN, _lib.FOLD_PLAIN, _lib.FOLD_QKV) or cout < 1 or per < 1 or (kind == _lib.FOLD_QKV and cout % 128):
            raise ValueError(f"fold_blob_table: record {i}: kind {kind}, cout {cout}, {per} elements per channel")
        plain = kind == _lib.FOLD_PLAIN
        if min(w_off, b_off) < 0 or (not plain and min(g_off, m_off, v_off) < 0):
            raise ValueError(f"fold_blob_table: record {i}: negative offset")
        tab[H + i * R:H + (i + 1) * R] = (w_off, 0 if plain else g_off, b_off, 0 if plain else m_off, 0 if plain else v_off, dst, cout | (per << 32),
                                          wg | (kind << 32))
        need[0], need[2] = max(need[0], w_off + cout * per), max(need[2], b_off + cout)
        if not plain:
            need[1], need[3] = max(need[1], g_off + cout), max(need[3], m_off + cout, v_off + cout)
        n = cout * (per + 1)
        dst, wg = dst + n, wg + (n + 255) // 256
    if wg >= 1 << 31:
        raise ValueError("fold_blob_table: too many workgroups for one launch")
    tab[:H] = (_lib.FOLD_MAGIC, len(recs), dst, *need, 0)
    return tab


def fold_blob_plan(device, records):
    """`fold_blob_table` on the device -> a `FoldTable`.  Once per net; synchronises (the table is copied to the device)."""
    tab = fold_blob_table(records)
    return FoldTable(torch.from_numpy(tab).to(device), tab, int(tab[1]), int(tab[2]), [int(v) for v in tab[3:7]])


def fold_blob_f32(w_flat, g_flat, b_flat, buffers, plan, eps=1e-3, out=None):
    """The fp32 data section of the "OBBW" blob of `plan` (a `FoldTable`) from the four flat buffers of a train.ParamGroups (or a ModelEMA's copies
    of them) by ONE kernel launch: BatchNorm folded into every conv in `train._BNBlock.fold()`'s fp32 operation order, the head's plain convs
    copied, the qkv rows back in checkpoint order.  No host read, copy or synchronisation: it can sit inside a captured graph."""
    srcs = [_chk(t, torch.float32, n) for t, n in zip((w_flat, g_flat, b_flat, buffers), ("w_flat", "g_flat", "b_flat", "buffers"))]
    for t, need, n in zip(srcs, plan.need, ("w_flat", "g_flat", "b_flat", "buffers")):
        if t.numel() < need or t.device != plan.table.device:
            raise ValueError(f"fold_blob_f32: {n} holds {t.numel()} elements on {t.device}, the plan reads {need} on {plan.table.device}")
    out = torch.empty(plan.out_elems, dtype=torch.float32, device=srcs[0].device) if out is None else _chk(out, torch.float32, "out")
    if out.numel() != plan.out_elems or out.device != plan.table.device:
        raise ValueError(f"fold_blob_f32: out holds {out.numel()} elements, the plan's data section {plan.out_elems}")
    _O.fold_blob(*srcs, plan.table, plan.nrec, float(eps), out)
    return out


def val_thresholds(device):
    """The validator's ten IoU thresholds, float32(linspace(0.5, 0.95, 10)), on the device"""
    return torch.linspace(0.5, 0.95, 10, dtype=torch.float32).to(device)


def val_match(det, count, gt_labels, gt_bboxes, mask_gt, nc, thr=None, out=None):
    """The validator's matching (csrc/valmatch.hip): det [B,max_det,7] / count [B] of `decode_nms`, the padded ground truth of `pad_targets` /
    `aug_labels` (pixels) -> (tp uint16 [B,max_det]: bit i = true positive at thr[i], best_iou fp32 [B,max_det], best_gt int32 [B,max_det], -1:
    none).  thr: device fp32, ascending, at most 16 (default `val_thresholds`).  Rows at or past count[b]: (0, 0, -1)."""
    d = _chk(det, torch.float32, "det")
    if d.dim() != 3 or d.shape[2] != 7 or d.shape[1] < 1:
        raise ValueError(f"val_match: det must be [B, max_det >= 1, 7], got {tuple(d.shape)}")
    B, max_det = d.shape[0], d.shape[1]
    cnt, gl, gb = _chk(count, torch.int32, "count"), _chk(gt_labels, torch.int32, "gt_labels"), _chk(gt_bboxes, torch.float32, "gt_bboxes")
    mk = mask_gt.view(torch.uint8) if mask_gt.dtype == torch.bool else mask_gt
    mk = _chk(mk, torch.uint8, "mask_gt")
    n_cap = gl.shape[1] if gl.dim() == 2 else 0
    if cnt.shape != (B,) or gl.shape != (B, n_cap) or gb.shape != (B, n_cap, 5) or mk.shape != (B, n_cap):
        raise ValueError("val_match: count [B], gt_labels [B,n_cap], gt_bboxes [B,n_cap,5], mask_gt [B,n_cap] expected")
    if not 1 <= n_cap <= _lib.VAL_MAX_GT or nc < 1:
        raise ValueError(f"val_match: n_cap = {n_cap} outside [1, {_lib.VAL_MAX_GT}] or nc = {nc} < 1")
    thr = val_thresholds(d.device) if thr is None else _chk(thr, torch.float32, "thr")
    if thr.dim() != 1 or not 1 <= thr.numel() <= _lib.VAL_MAX_THR:
        raise ValueError(f"val_match: 1..{_lib.VAL_MAX_THR} thresholds (one bit of tp each)")
    if out is None:
        out = (torch.empty((B, max_det), dtype=torch.uint16, device=d.device), torch.empty((B, max_det), dtype=torch.float32, device=d.device),
               torch.empty((B, max_det), dtype=torch.int32, device=d.device))
    tp, bi, bg = _chk(out[0], torch.uint16, "tp"), _chk(out[1], torch.float32, "best_iou"), _chk(out[2], torch.int32, "best_gt")
    if not (tp.shape == bi.shape == bg.shape == (B, max_det)):
        raise ValueError("val_match: out = (tp, best_iou, best_gt), each [B, max_det]")
    if B:
        _O.val_match(d, cnt, gl, gb, mk, int(nc), thr, tp, bi, bg)
    return tp, bi, bg


def _val_head_check(head, h, w, nc, fn):
    """the engine's head rows of an h x w input as obb_val_crit_* read them -> (B, A); ValueError otherwise"""
    hd = _chk(head, torch.float32, "head")
    if not 1 <= nc <= 64:
        raise ValueError(f"{fn}: nc = {nc}: 1..64")
    if h < 32 or w < 32 or h % 32 or w % 32:
        raise ValueError(f"{fn}: input {h} x {w}: h and w are positive multiples of 32")
    A, NO = sum((h // s) * (w // s) for s in (8, 16, 32)), (64 + nc + 1 + 3) // 4 * 4
    if hd.dim() != 3 or hd.shape[0] < 1 or tuple(hd.shape[1:]) != (A, NO):
        raise ValueError(f"{fn}: head must be [B >= 1, {A}, {NO}] for a {h} x {w} input with nc = {nc}, got {tuple(hd.shape)}")
    if hd.shape[0] * A * nc > 1 << 24:
        raise ValueError(f"{fn}: B A nc = {hd.shape[0] * A * nc} exceeds 2^24 elements")
    return hd.shape[0], A


def val_crit_decode(head, h, w, nc, out=None):
    """`crit_decode` on the engine's raw head rows (`forward`'s [B,A,NO] of an h x w input), read in place: -> (pd_scores [B,A,nc], pd_bboxes
    [B,A,5], anc_points [A,2], stride [A]), the same arithmetic -- bit-equal on equal logits.  csrc/valreport.hip; one launch."""
    B, A = _val_head_check(head, h, w, nc, "val_crit_decode")
    d = head.device
    if out is None:
        out = (torch.empty((B, A, nc), dtype=torch.float32, device=d), torch.empty((B, A, 5), dtype=torch.float32, device=d),
               torch.empty((A, 2), dtype=torch.float32, device=d), torch.empty((A,), dtype=torch.float32, device=d))
    ps, pb, ap, st = (_chk(t, torch.float32, n) for t, n in zip(out, ("pd_scores", "pd_bboxes", "anc_points", "stride")))
    if tuple(ps.shape) != (B, A, nc) or tuple(pb.shape) != (B, A, 5) or tuple(ap.shape) != (A, 2) or tuple(st.shape) != (A,):
        raise ValueError("val_crit_decode: out = (pd_scores [B,A,nc], pd_bboxes [B,A,5], anc_points [A,2], stride [A])")
    _O.val_crit_decode(head, int(h), int(w), int(nc), ps, pb, ap, st)
    return ps, pb, ap, st


def val_crit_items(head, h, w, nc, target_bboxes, target_scores, fg_mask, gains=(7.5, 0.5, 1.5), items=None, tss=None, accumulate=False):
    """`crit_loss` without the gradients, on the engine's raw head rows: -> (items fp32[3] = (box, cls, dfl) times their gains, tss fp32[1]).
    `accumulate` adds the three items to what `items` holds (a validation pass sums its batches on the device); fixed-order sums, no
    floating-point atomics: two runs give the same bits.  Nothing is read back to the host."""
    B, A = _val_head_check(head, h, w, nc, "val_crit_items")
    tb = _chk(target_bboxes, torch.float32, "target_bboxes")
    ts = _chk(target_scores, torch.float32, "target_scores")
    fg = fg_mask.view(torch.uint8) if fg_mask.dtype == torch.bool else fg_mask
    fg = _chk(fg, torch.uint8, "fg_mask")
    if tuple(tb.shape) != (B, A, 5) or tuple(ts.shape) != (B, A, nc) or tuple(fg.shape) != (B, A):
        raise ValueError(f"val_crit_items: targets {tuple(tb.shape)}, {tuple(ts.shape)}, {tuple(fg.shape)} do not match B = {B}, A = {A}, nc = {nc}")
    if len(gains) != 3:
        raise ValueError("val_crit_items: gains = (box, cls, dfl)")
    if accumulate and items is None:
        raise ValueError("val_crit_items: accumulate adds to `items`: pass the buffer")
    items = torch.empty(3, dtype=torch.float32, device=head.device) if items is None else _chk(items, torch.float32, "items")
    tss = torch.empty(1, dtype=torch.float32, device=head.device) if tss is None else _chk(tss, torch.float32, "tss")
    if items.numel() != 3 or tss.numel() != 1:
        raise ValueError("val_crit_items: items holds 3 values, tss 1")
    _O.val_crit_items(head, int(h), int(w), int(nc), tb, ts, fg, float(gains[0]), float(gains[1]), float(gains[2]), items, tss, bool(accumulate))
    return items, tss


def val_confusion(det, count, gt_labels, gt_bboxes, mask_gt, nc, conf_thr=0.25, iou_thr=0.45, matrix=None):
    """The validator's confusion matrix (csrc/valreport.hip; Ultralytics `ConfusionMatrix.process_batch` for OBB restated from recall, UNPINNED): the
    inputs of `val_match` -> matrix int32 [nc+1, nc+1], ADDED to (`matrix` None: a zeroed one): [pred, gt] per kept pair, [pred, nc] per
    detection above conf_thr without a ground truth, [nc, gt] per ground truth without a detection.  Class-agnostic ProbIoU > iou_thr; ties to
    the lower index.  Integer adds only."""
    d = _chk(det, torch.float32, "det")
    if d.dim() != 3 or d.shape[2] != 7 or d.shape[1] < 1:
        raise ValueError(f"val_confusion: det must be [B, max_det >= 1, 7], got {tuple(d.shape)}")
    B = d.shape[0]
    cnt, gl, gb = _chk(count, torch.int32, "count"), _chk(gt_labels, torch.int32, "gt_labels"), _chk(gt_bboxes, torch.float32, "gt_bboxes")
    mk = mask_gt.view(torch.uint8) if mask_gt.dtype == torch.bool else mask_gt
    mk = _chk(mk, torch.uint8, "mask_gt")
    n_cap = gl.shape[1] if gl.dim() == 2 else 0
    if cnt.shape != (B,) or gl.shape != (B, n_cap) or gb.shape != (B, n_cap, 5) or mk.shape != (B, n_cap):
        raise ValueError("val_confusion: count [B], gt_labels [B,n_cap], gt_bboxes [B,n_cap,5], mask_gt [B,n_cap] expected")
    if not 1 <= n_cap <= _lib.VAL_MAX_GT or not 1 <= nc <= 32766:
        raise ValueError(f"val_confusion: n_cap = {n_cap} outside [1, {_lib.VAL_MAX_GT}] or nc = {nc} outside [1, 32766]")
    if conf_thr != conf_thr or iou_thr != iou_thr:
        raise ValueError("val_confusion: a NaN threshold")
    matrix = torch.zeros((nc + 1, nc + 1), dtype=torch.int32, device=d.device) if matrix is None else _chk(matrix, torch.int32, "matrix")
    if tuple(matrix.shape) != (nc + 1, nc + 1):
        raise ValueError(f"val_confusion: matrix must be [{nc + 1}, {nc + 1}]")
    if B:
        _O.val_confusion(d, cnt, gl, gb, mk, int(nc), float(conf_thr), float(iou_thr), matrix)
    return matrix


def dfl_loss(pred_dist, target_ltrb, weight=None, target_scores_sum=1.0, reg_max=16):
    """DFL term of the OBB loss for n matched anchors, forward + backward in one launch: pred_dist [n, 4*reg_max] (or [n*4, reg_max]) logits,
    target_ltrb [n,4] distances in bins, weight [n] or None -> (loss float32[1], grad [n, 4*reg_max]).  ultralytics DFLoss / RotatedBboxLoss."""
    t = _chk(target_ltrb, torch.float32, "target_ltrb").reshape(-1, 4)
    p = _chk(pred_dist, torch.float32, "pred_dist").reshape(t.shape[0], 4 * reg_max)
    if weight is not None:
        weight = _chk(weight, torch.float32, "weight").reshape(-1)
        if weight.shape[0] != t.shape[0]:
            raise ValueError("dfl_loss: weight length mismatch")
    loss = torch.zeros(1, dtype=torch.float32, device=p.device)
    grad = torch.empty_like(p)
    _O.dfl_loss(p, t, weight, int(reg_max), float(target_scores_sum), loss, grad)
    return loss, grad


def bce_loss(logits, targets, target_scores_sum=1.0):
    """Classification term of the OBB loss: BCEWithLogits(reduction none)(logits, targets).sum() / target_scores_sum, forward + backward in
    one launch: logits, targets float32 of equal shape -> (loss float32[1], grad like logits)."""
    x = _chk(logits, torch.float32, "logits")
    t = _chk(targets, torch.float32, "targets")
    if x.shape != t.shape:
        raise ValueError("bce_loss: shape mismatch")
    loss = torch.zeros(1, dtype=torch.float32, device=x.device)
    grad = torch.empty_like(x)
    _O.bce_loss(x, t, float(target_scores_sum), loss, grad)
    return loss, grad


def _crit_check(box, cls, angle, fn):
    """the head's three levels as obb_crit_* read them -> (B, nc, A); ValueError otherwise"""
    if not (len(box) == len(cls) == len(angle) == 3):
        raise ValueError(f"{fn}: box, cls and angle are lists of three levels (P3, P4, P5)")
    if box[0].dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"{fn}: box logits are bf16 or fp32, got {box[0].dtype}")
    B, nc, A = box[0].shape[0], cls[0].shape[-1], 0
    if not 1 <= nc <= 64:
        raise ValueError(f"{fn}: nc = {nc}: 1..64")
    for i, (b, c, a) in enumerate(zip(box, cls, angle)):
        _chk(b, box[0].dtype, f"box[{i}]"); _chk(c, torch.float32, f"cls[{i}]"); _chk(a, torch.float32, f"angle[{i}]")
        if b.dim() != 4 or b.shape[0] != B or b.shape[3] != 64 or min(b.shape[1:3]) < 1:
            raise ValueError(f"{fn}: box[{i}] must be [B,H,W,64] with H, W >= 1, got {tuple(b.shape)}")
        if tuple(c.shape) != (*b.shape[:3], nc) or tuple(a.shape) != (*b.shape[:3], 1):
            raise ValueError(f"{fn}: level {i}: cls {tuple(c.shape)} / angle {tuple(a.shape)} do not match box {tuple(b.shape)} with nc = {nc}")
        A += b.shape[1] * b.shape[2]
    if B * A * nc > 1 << 24:
        raise ValueError(f"{fn}: B A nc = {B * A * nc} exceeds the sum tree's 2^24 elements")
    return B, nc, A


def crit_decode(box, cls, angle):
    """Training-mode decode of the head (v8OBBLoss.__call__ up to the assigner; restated from recall, parity unpinned): box / cls / angle = lists
    of the three levels' logits ([B,H,W,64] bf16 or fp32; [B,H,W,nc] fp32; [B,H,W,1] fp32) -> (pd_scores [B,A,nc] = sigmoid(cls), pd_bboxes
    [B,A,5] xywh in pixels + theta, anc_points [A,2] in pixels, stride [A]), fp32: the inputs of `rotated_tal_assign`.  One launch."""
    B, nc, A = _crit_check(box, cls, angle, "crit_decode")
    d = box[0].device
    ps = torch.empty((B, A, nc), dtype=torch.float32, device=d)
    pb = torch.empty((B, A, 5), dtype=torch.float32, device=d)
    ap = torch.empty((A, 2), dtype=torch.float32, device=d)
    st = torch.empty((A,), dtype=torch.float32, device=d)
    _O.crit_decode(*box, *cls, *angle, ps, pb, ap, st)
    return ps, pb, ap, st


def crit_loss(box, cls, angle, target_bboxes, target_scores, fg_mask, gains=(7.5, 0.5, 1.5), out=None):
    """The three terms of v8OBBLoss and the gradient of every head logit, given the assignment (restated from recall, parity unpinned):
    target_bboxes [B,A,5] (pixels), target_scores [B,A,nc], fg_mask [B,A] as `rotated_tal_assign` returns them -> (items fp32[3] = (box, cls, dfl)
    times their gains, tss fp32[1] = max(sum target_scores, 1), d_box list (bf16, like box), d_cls list, d_angle list (fp32)): the gradients of
    B * sum(items), every element written.  `out` = (d_box, d_cls, d_angle) writes into the caller's buffers.  Nothing is read back to the host."""
    B, nc, A = _crit_check(box, cls, angle, "crit_loss")
    tb = _chk(target_bboxes, torch.float32, "target_bboxes")
    ts = _chk(target_scores, torch.float32, "target_scores")
    fg = fg_mask.view(torch.uint8) if fg_mask.dtype == torch.bool else fg_mask
    fg = _chk(fg, torch.uint8, "fg_mask")
    if tuple(tb.shape) != (B, A, 5) or tuple(ts.shape) != (B, A, nc) or tuple(fg.shape) != (B, A):
        raise ValueError(f"crit_loss: targets {tuple(tb.shape)}, {tuple(ts.shape)}, {tuple(fg.shape)} do not match B = {B}, A = {A}, nc = {nc}")
    if len(gains) != 3:
        raise ValueError("crit_loss: gains = (box, cls, dfl)")
    d = box[0].device
    if out is None:
        d_box = [torch.empty(b.shape, dtype=torch.bfloat16, device=d) for b in box]
        d_cls = [torch.empty_like(c) for c in cls]
        d_angle = [torch.empty_like(a) for a in angle]
    else:
        d_box, d_cls, d_angle = out
        for i in range(3):
            _chk(d_box[i], torch.bfloat16, f"d_box[{i}]"); _chk(d_cls[i], torch.float32, f"d_cls[{i}]"); _chk(d_angle[i], torch.float32, f"d_angle[{i}]")
            if d_box[i].shape != box[i].shape or d_cls[i].shape != cls[i].shape or d_angle[i].shape != angle[i].shape:
                raise ValueError(f"crit_loss: out buffers of level {i} do not match the logits' shapes")
    items = torch.empty(3, dtype=torch.float32, device=d)
    tss = torch.empty(1, dtype=torch.float32, device=d)
    _O.crit_loss(*box, *cls, *angle, tb, ts, fg, float(gains[0]), float(gains[1]), float(gains[2]), *d_box, *d_cls, *d_angle, items, tss)
    return items, tss, list(d_box), list(d_cls), list(d_angle)


def sgd_step(param, grad, momentum_buf, lr, momentum=0.9, weight_decay=0.0, nesterov=True, first_step=False):
    """In place, one launch: torch.optim.SGD's update (dampening 0) of a flat fp32 parameter group; `first_step` initialises the momentum
    buffer with the (decayed) gradient as torch does."""
    p, g, b = _chk(param, torch.float32, "param"), _chk(grad, torch.float32, "grad"), _chk(momentum_buf, torch.float32, "momentum_buf")
    if not (p.numel() == g.numel() == b.numel()):
        raise ValueError("sgd_step: size mismatch")
    _O.sgd_step(p, g, b, float(lr), float(momentum), float(weight_decay), bool(nesterov), bool(first_step))


def adamw_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """In place, one launch: torch.optim.AdamW's update of a flat fp32 parameter group; `step` counts from 1."""
    p, g = _chk(param, torch.float32, "param"), _chk(grad, torch.float32, "grad")
    m, v = _chk(exp_avg, torch.float32, "exp_avg"), _chk(exp_avg_sq, torch.float32, "exp_avg_sq")
    if not (p.numel() == g.numel() == m.numel() == v.numel()):
        raise ValueError("adamw_step: size mismatch")
    _O.adamw_step(p, g, m, v, int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))


MAX_SEGMENTS = 8  # segments per launch of the trainer-update kernels (csrc/trainupd.hip: kMaxSeg)


def _seg_lists(name, first, *others):
    """flat fp32 segment lists of one call: at most MAX_SEGMENTS, every list as long as the first and element for element the same size"""
    first = [_chk(t, torch.float32, f"{name}[{i}]").reshape(-1) for i, t in enumerate(first)]
    if not 1 <= len(first) <= MAX_SEGMENTS:
        raise ValueError(f"{name}: 1 to {MAX_SEGMENTS} segments, got {len(first)}")
    out = [first]
    for o in others:
        o = [_chk(t, torch.float32, f"{name}[{i}]").reshape(-1) for i, t in enumerate(o)]
        if [t.numel() for t in o] != [t.numel() for t in first]:
            raise ValueError(f"{name}: the segment lists differ in length or sizes")
        out.append(o)
    return out


def _per_segment(v, k, name):
    v = [float(v)] * k if isinstance(v, (int, float)) else [float(x) for x in v]
    if len(v) != k:
        raise ValueError(f"{name}: one value or one per segment ({k}), got {len(v)}")
    return v


def sumsq_partials(sizes):
    """How many double partials `grad_sumsq` writes for segments of these sizes (one per 4096-element slab of each)."""
    n = (C.c_int64 * len(sizes))(*[int(s) for s in sizes])
    count = C.c_int64(0)
    if _lib.lib().obb_grad_sumsq_partials(n, len(sizes), C.byref(count)) != 0:
        raise ValueError(f"sumsq_partials: at most {MAX_SEGMENTS} segments of non-negative size")
    return count.value


def grad_sumsq(grads, partials=None):
    """One launch over a list of flat fp32 gradient buffers -> partials fp64[sumsq_partials(sizes)]: the sum of squares of every 4096-element slab,
    squares and sums in double (exact per square; 1e20 and 1e-25 neither overflow nor vanish), reduced in a fixed order: reproducible."""
    (g,) = _seg_lists("grad_sumsq", grads)
    need = sumsq_partials([t.numel() for t in g])
    if partials is None:
        partials = torch.empty(need, dtype=torch.float64, device=g[0].device)
    elif _chk(partials, torch.float64, "partials").numel() != need:
        raise ValueError(f"grad_sumsq: partials must hold {need} doubles")
    _O.grad_sumsq(g, partials)
    return partials


def clip_coef(partials, max_norm=10.0, clip=None):
    """One launch, one workgroup: the partials of `grad_sumsq` -> clip fp32[3] ON THE DEVICE = (total_norm, coef = min(1, max_norm / (total_norm + 1e-6)),
    finite) -- torch.nn.utils.clip_grad_norm_'s coefficient (NaN norm: NaN; infinite norm: 0) without its host read."""
    pt = _chk(partials, torch.float64, "partials")
    if clip is None:
        clip = torch.empty(3, dtype=torch.float32, device=pt.device)
    elif _chk(clip, torch.float32, "clip").numel() != 3:
        raise ValueError("clip_coef: clip is fp32[3]")
    _O.clip_coef(pt, float(max_norm), clip)
    return clip


def clip_grad_norm(grads, max_norm=10.0):
    """torch.nn.utils.clip_grad_norm_ over flat gradient buffers in two launches, WITHOUT touching the gradients and without a host read: -> clip
    fp32[3] on the device (see `clip_coef`); `sgd_step_multi` / `adamw_step_multi` apply clip[1] as they read the gradients."""
    return clip_coef(grad_sumsq(grads), max_norm)


def _clip_arg(clip):
    if clip is not None and _chk(clip, torch.float32, "clip").numel() != 3:
        raise ValueError("clip is the fp32[3] device tensor of clip_coef")
    return clip


def sgd_step_multi(params, grads, momentum_bufs, lr, momentum=0.9, weight_decay=0.0, nesterov=True, first_step=False, clip=None):
    """In place, ONE launch for all groups: `sgd_step` of every (param, grad, momentum_buf) with its own lr and weight_decay (a number, or one per
    group) on the gradient times clip[1] (clip = None: as it is).  Bit-identical to `sgd_step` per group when clip[1] == 1 or clip is None."""
    p, g, b = _seg_lists("sgd_step_multi", params, grads, momentum_bufs)
    _O.sgd_step_multi(p, g, b, _per_segment(lr, len(p), "lr"), _per_segment(weight_decay, len(p), "weight_decay"), float(momentum), bool(nesterov),
                      bool(first_step), _clip_arg(clip))


def adamw_step_multi(params, grads, exp_avgs, exp_avg_sqs, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip=None):
    """In place, ONE launch for all groups: `adamw_step` of every group with its own lr and weight_decay on the gradient times clip[1]; `step` counts
    from 1.  Bit-identical to `adamw_step` per group when clip[1] == 1 or clip is None."""
    p, g, m, v = _seg_lists("adamw_step_multi", params, grads, exp_avgs, exp_avg_sqs)
    _O.adamw_step_multi(p, g, m, v, _per_segment(lr, len(p), "lr"), _per_segment(weight_decay, len(p), "weight_decay"), int(step), float(betas[0]),
                        float(betas[1]), float(eps), _clip_arg(clip))


def grad_accumulate(accs, grads, first=False):
    """In place, one launch: acc = first ? grad : acc + grad for every pair of flat buffers (`first`: acc is not read)."""
    a, g = _seg_lists("grad_accumulate", accs, grads)
    _O.grad_accumulate(a, g, bool(first))


def ema_update(emas, srcs, decay):
    """In place, one launch: ema = ema * d + (1 - d) * src for every pair of flat buffers, in the operation order of ultralytics ModelEMA.update
    (mul_, then add_ of the scaled source); d and 1 - d are each rounded to fp32 from the double `decay`."""
    e, s = _seg_lists("ema_update", emas, srcs)
    _O.ema_update(e, s, float(decay))


def probiou_loss(pred, target, weight=None, target_scores_sum=1.0):
    """ProbIoU rotated-box loss of n matched pairs, forward + backward in one launch: pred, target [n,5] (x,y,w,h,theta) float32,
    weight [n] or None -> (loss float32[1], grad_pred [n,5] = d loss / d pred).  Train_OBB.py:796-841 -> v8OBBLoss / RotatedBboxLoss."""
    p = _chk(pred, torch.float32, "pred").reshape(-1, 5)
    t = _chk(target, torch.float32, "target").reshape(-1, 5)
    if p.shape != t.shape:
        raise ValueError("probiou_loss: shape mismatch")
    if weight is not None:
        weight = _chk(weight, torch.float32, "weight").reshape(-1)
        if weight.shape[0] != p.shape[0]:
            raise ValueError("probiou_loss: weight length mismatch")
    loss = torch.zeros(1, dtype=torch.float32, device=p.device)
    grad = torch.empty_like(p)
    _O.probiou_loss(p, t, weight, float(target_scores_sum), loss, grad)
    return loss, grad
