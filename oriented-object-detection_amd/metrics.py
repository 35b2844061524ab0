"""The mAP instrument of Detect_OBB.py (row a15 of SURVEY.md section 8) on the GPU polygon-IoU kernel:

    _load_gt_as_pixels        :436-454   (labels: `cls x1 y1 ... x4 y4` normalised -> pixels; image size passed in, no cv2)
    gather_detections_and_gts :501-510
    compute_pr_for_class      :512-565   (score-ordered greedy matching, strict `iou > best_iou`, then `best_iou >= thr`)
    compute_ap_from_pr        :489-499   (all-point interpolation)
    evaluate_map              :574-607   (mean over GT-present classes, classes without detections count as AP 0)

All detection x ground-truth IoUs of one (class, image) pair come from one obb_poly_iou_matrix launch; the greedy matching is the
reference's own sequential loop over that matrix (control flow, no arithmetic)."""
import numpy as np
import torch

from . import ops

MAP_MIN_SCORE = 0.001  # Detect_OBB.py:34


def load_gt_as_pixels(label_path, w, h):
    gts = []
    with open(label_path, "r") as f:
        for line in f:
            parts = line.strip().split()
            if len(parts) != 9:
                continue
            vals = list(map(float, parts[1:]))
            pts = [c for i in range(0, 8, 2) for c in (vals[i] * w, vals[i + 1] * h)]
            gts.append({"cls": int(parts[0]), "pts": pts})
    return gts


def compute_ap_from_pr(recall, precision):
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([0.0], precision, [0.0]))
    for i in range(mpre.size - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    idx = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[idx + 1] - mrec[idx]) * mpre[idx + 1]))


def compute_pr_for_class(dets, gts, iou_thr=0.5, device=None):
    """dets: list of {"image_id", "score", "bbox"(8)}; gts: {image_id: [bbox8, ...]} -> (precision, recall, ap, TP, FP, FN)"""
    npos = sum(len(v) for v in gts.values())
    if npos == 0:
        return np.array([0.0]), np.array([0.0]), 0.0, 0, 0, 0
    dets_sorted = sorted(dets, key=lambda x: x["score"], reverse=True)
    if len(dets_sorted) == 0:
        return np.array([0.0]), np.array([0.0]), 0.0, 0, 0, npos
    dev = device or torch.device("cuda", torch.cuda.current_device())
    # one IoU matrix per image (detections of that image x its ground truths)
    by_img = {}
    for i, d in enumerate(dets_sorted):
        by_img.setdefault(d["image_id"], []).append(i)
    iou_rows = {}
    for img, idxs in by_img.items():
        g = gts.get(img, [])
        if not g:
            continue
        a = torch.tensor([list(dets_sorted[i]["bbox"][:8]) for i in idxs], dtype=torch.float64, device=dev)
        b = torch.tensor([list(x) for x in g], dtype=torch.float64, device=dev)
        m = ops.poly_iou_matrix(a, b).cpu().numpy()
        for r, i in enumerate(idxs):
            iou_rows[i] = m[r]
    tp, fp = np.zeros(len(dets_sorted)), np.zeros(len(dets_sorted))
    matched = {img: np.zeros(len(v), dtype=bool) for img, v in gts.items()}
    for i, det in enumerate(dets_sorted):
        img = det["image_id"]
        best_iou, best_j = 0.0, -1
        row = iou_rows.get(i)
        if row is not None:
            for j in range(len(row)):
                if matched[img][j]:
                    continue
                if row[j] > best_iou:
                    best_iou, best_j = row[j], j
        if best_iou >= iou_thr and best_j >= 0:
            tp[i] = 1
            matched[img][best_j] = True
        else:
            fp[i] = 1
    tp_cum, fp_cum = np.cumsum(tp), np.cumsum(fp)
    recall = tp_cum / (npos + 1e-9)
    precision = tp_cum / (tp_cum + fp_cum + 1e-9)
    ap = compute_ap_from_pr(recall, precision)
    return precision, recall, ap, int(tp_cum[-1]), int(fp_cum[-1]), npos - int(tp_cum[-1])


def gather_detections_and_gts(dets_source, gt_source, cls_id):
    dets, gts = [], {}
    for img, gt_boxes in gt_source.items():
        for d in dets_source.get(img, []):
            if int(d[8]) == cls_id and d[9] >= MAP_MIN_SCORE:
                dets.append({"image_id": img, "score": float(d[9]), "bbox": d[:8]})
        gts[img] = [g["pts"] for g in gt_boxes if g["cls"] == cls_id]
    return dets, gts


def evaluate_map(dets_source, gt_source, iou_list=None):
    """dets_source: {image: [11-tuples]}, gt_source: {image: [{"cls", "pts"}]} -> the reference's result dict"""
    if iou_list is None:
        iou_list = [0.5] + [round(0.5 + 0.05 * i, 2) for i in range(1, 10)]
    class_ids = sorted({int(g["cls"]) for gl in gt_source.values() for g in gl})
    per_iou = {}
    for iou in iou_list:
        aps = []
        for cid in class_ids:
            dets, gts = gather_detections_and_gts(dets_source, gt_source, cid)
            aps.append(compute_pr_for_class(dets, gts, iou_thr=iou)[2])
        per_iou[iou] = float(np.mean(aps)) if aps else 0.0
    return {"mAP@0.5": per_iou.get(0.5, 0.0), "mAP@[0.5:0.95]": float(np.mean([per_iou[i] for i in iou_list])) if iou_list else 0.0,
            "per_iou": per_iou}


# ---------------------------------------------------------------------------------------------------------------------------
# The TRAINER's AP (the `val` pass behind every epoch of `model.train(...)`, Train_OBB.py:792-841): Ultralytics 8.3.x `ap_per_class` / `compute_ap`,
# restated from recall (the package is not installed: UNPINNED, like train.Schedule).  Another instrument than the one above: ProbIoU matches at ten
# thresholds (train.Validator / ops.val_match produce them on the device) and a 101-point interpolated AP, where Detect_OBB.py's uses polygon IoU,
# one threshold and the all-point AP.  Both stay.

def compute_ap(recall, precision):
    """AP of one precision / recall curve (numpy float64, in confidence order): sentinels mrec = [0, r, 1], mpre = [1, p, 0], the precision envelope
    (running maximum from the right), then the trapezoid rule over interp(linspace(0, 1, 101), mrec, mpre) -- COCO's 101 points."""
    mrec = np.concatenate(([0.0], np.asarray(recall, np.float64), [1.0]))
    mpre = np.concatenate(([1.0], np.asarray(precision, np.float64), [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    x = np.linspace(0.0, 1.0, 101)
    y = np.interp(x, mrec, mpre)
    return float(np.sum((y[1:] + y[:-1]) * 0.5 * (x[1:] - x[:-1])))


def ap_per_class(tp, conf, pred_cls, target_cls, nc):
    """tp bool [n, T] (true positive of detection d at threshold t: `ops.val_match`'s bits), conf [n], pred_cls [n], target_cls [m] (the class of
    every ground truth), classes in [0, nc) -> {"ap": float64 [classes present in the targets, T], "classes": those classes, "map50": mean of
    column 0, "map": mean of all, "fitness": 0.1 map50 + 0.9 map}.  Detections are put in descending confidence by a STABLE sort (equal
    confidences keep their input order); per class present in the targets: cumulative TP and FP per threshold, recall = tpc / (n_gt + 1e-16),
    precision = tpc / (tpc + fpc), `compute_ap`.  A class with targets and no detections scores 0; detections of a class without targets
    count nowhere; no targets at all: every figure 0.  A perfect detector scores 0.995, not 1: the envelope's last sentinel pulls the 101st
    point to 0."""
    tp = np.asarray(tp).astype(bool)
    if tp.ndim != 2:
        raise ValueError("ap_per_class: tp must be [n, thresholds]")
    conf, pred_cls, target_cls = np.asarray(conf, np.float64).reshape(-1), np.asarray(pred_cls).reshape(-1), np.asarray(target_cls).reshape(-1)
    if len(conf) != len(tp) or len(pred_cls) != len(tp):
        raise ValueError("ap_per_class: tp, conf and pred_cls differ in length")
    if len(target_cls) and (target_cls.min() < 0 or target_cls.max() >= nc):
        raise ValueError(f"ap_per_class: a target class outside [0, {nc})")
    order = np.argsort(-conf, kind="stable")
    tp, pred_cls = tp[order], pred_cls[order]
    classes, n_gt = np.unique(target_cls.astype(np.int64), return_counts=True)
    ap = np.zeros((len(classes), tp.shape[1]))
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        if not sel.any():
            continue
        tpc = tp[sel].cumsum(0).astype(np.float64)
        fpc = (~tp[sel]).cumsum(0).astype(np.float64)
        recall, precision = tpc / (n_gt[ci] + 1e-16), tpc / (tpc + fpc)
        for j in range(tp.shape[1]):
            ap[ci, j] = compute_ap(recall[:, j], precision[:, j])
    map50 = float(ap[:, 0].mean()) if ap.size else 0.0
    mean = float(ap.mean()) if ap.size else 0.0
    return {"ap": ap, "classes": classes, "map50": map50, "map": mean, "fitness": 0.1 * map50 + 0.9 * mean}


def smooth_box(y, f=0.1):
    """Ultralytics' `smooth(y, f)`: a box filter of nf = round(2 f len(y)) // 2 + 1 taps (101 for 1000 points and f = 0.1) over y padded by nf // 2
    copies of its first and of its last value -> the same length"""
    y = np.asarray(y, np.float64)
    nf = round(len(y) * f * 2) // 2 + 1
    yp = np.concatenate((np.full(nf // 2, y[0]), y, np.full(nf // 2, y[-1])))
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def pr_curves(tp, conf, pred_cls, target_cls, nc):
    """The P / R / F1 curves over confidence and the operating point the trainer reports as `metrics/precision` / `metrics/recall` (the curve half
    of Ultralytics 8.3.x `ap_per_class`, restated from recall: the package is not installed, UNPINNED like `ap_per_class` above).  Arguments as
    `ap_per_class`; column 0 of tp (IoU 0.5) is read, the detections go through the same stable sort.  x = linspace(0, 1, 1000); per class present
    in the targets, with conf_c / recall / precision its detections' confidences and cumulative curves: r = interp(-x, -conf_c, recall, left=0),
    p = interp(-x, -conf_c, precision, left=1) (below the least confidence: the last value; among equal confidences numpy reads the LAST of
    them, the state after all of the tie), f1 = 2 p r / (p + r + 1e-16).  The operating index is the argmax of the class-mean F1 smoothed by
    `smooth_box` (101 taps).  -> {"x", "p_curve", "r_curve", "f1_curve" [classes present, 1000], "classes", "conf_best" = x[index], "p", "r", "f1"
    [classes present] at the index, "mp", "mr" their means}.  A class with targets and no detections scores 0 on all three curves; no targets
    at all: empty curves, every figure and conf_best 0."""
    tp = np.asarray(tp).astype(bool)
    if tp.ndim != 2 or tp.shape[1] < 1:
        raise ValueError("pr_curves: tp must be [n, thresholds >= 1]")
    conf, pred_cls, target_cls = np.asarray(conf, np.float64).reshape(-1), np.asarray(pred_cls).reshape(-1), np.asarray(target_cls).reshape(-1)
    if len(conf) != len(tp) or len(pred_cls) != len(tp):
        raise ValueError("pr_curves: tp, conf and pred_cls differ in length")
    if len(target_cls) and (target_cls.min() < 0 or target_cls.max() >= nc):
        raise ValueError(f"pr_curves: a target class outside [0, {nc})")
    order = np.argsort(-conf, kind="stable")
    tp0, conf, pred_cls = tp[order, 0], conf[order], pred_cls[order]
    classes, n_gt = np.unique(target_cls.astype(np.int64), return_counts=True)
    x = np.linspace(0.0, 1.0, 1000)
    p_curve, r_curve = np.zeros((len(classes), x.size)), np.zeros((len(classes), x.size))
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        if not sel.any():
            continue
        tpc = tp0[sel].cumsum().astype(np.float64)
        fpc = (~tp0[sel]).cumsum().astype(np.float64)
        r_curve[ci] = np.interp(-x, -conf[sel], tpc / (n_gt[ci] + 1e-16), left=0.0)
        p_curve[ci] = np.interp(-x, -conf[sel], tpc / (tpc + fpc), left=1.0)
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + 1e-16)
    i = int(np.argmax(smooth_box(f1_curve.mean(0), 0.1))) if len(classes) else 0
    p, r, f1 = p_curve[:, i], r_curve[:, i], f1_curve[:, i]
    return {"x": x, "p_curve": p_curve, "r_curve": r_curve, "f1_curve": f1_curve, "classes": classes, "conf_best": float(x[i]) if len(classes) else 0.0,
            "p": p, "r": r, "f1": f1, "mp": float(p.mean()) if len(classes) else 0.0, "mr": float(r.mean()) if len(classes) else 0.0}


# ---------------------------------------------------------------------------------------------------------------------------
# Fusion-evaluation metrics beyond mAP.  dets: 11-tuples (x1..y4, cls, conf, angle) in pixels;
# gts: [{"cls": int, "pts": 8 floats}].  All geometry runs on the GPU (one matrix launch per image); the greedy matching loops are
# the reference's own sequential control flow over those matrices.

def prec_rec_f1(tp, fp, fn):
    """Detect_OBB.py:482-486"""
    P = tp / (tp + fp + 1e-9)
    R = tp / (tp + fn + 1e-9)
    return P, R, 2 * P * R / (P + R + 1e-9)


def _dev(device):
    return device or torch.device("cuda", torch.cuda.current_device())


def match_dets_to_gts_pixel(dets, gts, iou_thr=0.5, device=None):
    """Detect_OBB.py:456-480: detections in LIST order (no score sort), strict `iou > best_iou`, then `best_iou >= thr` -> (TP, FP, FN)"""
    if not dets or not gts:
        return 0, len(dets), len(gts)
    dev = _dev(device)
    a = torch.tensor([list(d[:8]) for d in dets], dtype=torch.float64, device=dev)
    b = torch.tensor([list(g["pts"]) for g in gts], dtype=torch.float64, device=dev)
    ca = torch.tensor([int(d[8]) for d in dets], dtype=torch.int32, device=dev)
    cb = torch.tensor([int(g["cls"]) for g in gts], dtype=torch.int32, device=dev)
    iou = ops.poly_iou_matrix(a, b, ca, cb).cpu().numpy()  # 0 where the classes differ
    same = ca.cpu().numpy()[:, None] == cb.cpu().numpy()[None, :]
    used = np.zeros(len(gts), bool)
    tp = 0
    for i in range(len(dets)):
        best_iou, best_j = 0.0, -1
        row = iou[i]
        for j in np.nonzero(same[i] & ~used)[0]:
            if row[j] > best_iou:
                best_iou, best_j = row[j], j
        if best_iou >= iou_thr and best_j >= 0:
            used[best_j] = True
            tp += 1
    return tp, len(dets) - tp, int((~used).sum())


def center_hit_counts(dets, gts, device=None):
    """body of evaluate_center_hit (:609-648) for one image -> (TP, FP, FN)"""
    if not dets or not gts:
        return 0, len(dets), len(gts)
    dev = _dev(device)
    bx = np.array([list(d[:8]) for d in dets], np.float64)
    ctr = np.stack([(bx[:, 0] + bx[:, 2] + bx[:, 4] + bx[:, 6]) / 4.0, (bx[:, 1] + bx[:, 3] + bx[:, 5] + bx[:, 7]) / 4.0], 1)  # :159-165
    inside = ops.points_in_quads(torch.as_tensor(ctr, device=dev), torch.tensor([list(g["pts"]) for g in gts], dtype=torch.float64, device=dev),
                                 torch.tensor([int(d[8]) for d in dets], dtype=torch.int32, device=dev),
                                 torch.tensor([int(g["cls"]) for g in gts], dtype=torch.int32, device=dev)).cpu().numpy().astype(bool)
    used = np.zeros(len(gts), bool)
    tp = fp = 0
    for i in range(len(dets)):
        cand = np.nonzero(inside[i] & ~used)[0]
        if len(cand):  # first unused, same-class, valid GT polygon that contains the centre
            used[cand[0]] = True
            tp += 1
        else:
            fp += 1
    return tp, fp, int((~used).sum())


def evaluate_center_hit(dets_source, gt_source, conf_thr=0.5, device=None):
    """-> (P, R, F1, TP, FP, FN)"""
    tp = fp = fn = 0
    for img, gts in gt_source.items():
        dets = [d for d in dets_source.get(img, []) if d[9] >= conf_thr]
        a, b, c = center_hit_counts(dets, gts, device)
        tp += a; fp += b; fn += c
    return prec_rec_f1(tp, fp, fn) + (tp, fp, fn)


def evaluate_dataset(dets_source, gt_source, conf_thr, iou_thr, device=None):
    """Detect_OBB.py:650-658 -> (P, R, F1)"""
    tp = fp = fn = 0
    for img, gts in gt_source.items():
        filtered = [d for d in dets_source.get(img, []) if d[9] >= conf_thr]
        a, b, c = match_dets_to_gts_pixel(filtered, gts, iou_thr, device)
        tp += a; fp += b; fn += c
    return prec_rec_f1(tp, fp, fn)


def classwise_report(dets_source, gt_source, conf_thr, iou_thr, class_names=None, csv_path=None, device=None):
    """Detect_OBB.py:660-686: rows [cls_id, class, TP, FP, FN, Precision, Recall, F1] for every class that has a detection
    (CSV instead of the reference's xlsx when csv_path is given)."""
    cids = sorted({int(d[8]) for dets in dets_source.values() for d in dets})
    rows = []
    for cid in cids:
        tp = fp = fn = 0
        for img, gts in gt_source.items():
            dets_c = [d for d in dets_source.get(img, []) if int(d[8]) == cid and d[9] >= conf_thr]
            a, b, c = match_dets_to_gts_pixel(dets_c, [g for g in gts if g["cls"] == cid], iou_thr, device)
            tp += a; fp += b; fn += c
        rows.append([cid, (class_names or {}).get(cid, str(cid)), tp, fp, fn, *prec_rec_f1(tp, fp, fn)])
    if csv_path:
        with open(csv_path, "w") as f:
            f.write("cls_id,class,TP,FP,FN,Precision,Recall,F1\n")
            for r in rows:
                f.write(",".join(str(v) for v in r) + "\n")
    return rows


def run_fusion_eval(dets_source, gt_source, iou_thr=0.25, class_names=None, csv_path=None, verbose=True, device=None):
    """Detect_OBB.py:688-741 (the single-scale and the dual-scale branch report the same quantities): the reference uses `iou_thr`
    (:36, 0.25) BOTH as the confidence threshold of the P/R/F1, class-wise and Center-Hit reports and as their IoU threshold.
    dets_source: {image: [11-tuples]} (what process_image stores in all_dets_per_image, :344-345); gt_source: {image: [{"cls", "pts"}]}.
    -> dict with every number the reference prints."""
    thr = float(iou_thr)
    out = {"conf_thr": thr, "iou_thr": float(iou_thr)}
    P, R, F1 = evaluate_dataset(dets_source, gt_source, conf_thr=thr, iou_thr=iou_thr, device=device)
    out["precision"], out["recall"], out["f1"] = P, R, F1
    out["classwise"] = classwise_report(dets_source, gt_source, conf_thr=thr, iou_thr=iou_thr, class_names=class_names, csv_path=csv_path, device=device)
    ch = evaluate_center_hit(dets_source, gt_source, conf_thr=thr, device=device)
    out["center_hit"] = {"P": ch[0], "R": ch[1], "F1": ch[2], "TP": ch[3], "FP": ch[4], "FN": ch[5]}
    maps = evaluate_map(dets_source, gt_source, iou_list=list(np.arange(0.5, 0.96, 0.05)))
    out["mAP@0.5"], out["mAP@[0.5:0.95]"] = maps["mAP@0.5"], maps["mAP@[0.5:0.95]"]
    soft_list = [0.30, 0.40, 0.50, 0.60, 0.70]
    maps_soft = evaluate_map(dets_source, gt_source, iou_list=soft_list)
    out["mAP@0.3"] = maps_soft["per_iou"][0.30]
    out["mAP@[0.3:0.7]"] = float(np.mean([maps_soft["per_iou"][i] for i in soft_list]))
    if verbose:
        print(f"[Report @ {thr:.2f}] Precision={P:.3f} | Recall={R:.3f} | F1={F1:.3f}")
        print(f"[Center-Hit @ conf≥{thr:.2f}] P={ch[0]:.3f} R={ch[1]:.3f} F1={ch[2]:.3f} (TP={ch[3]}, FP={ch[4]}, FN={ch[5]})")
        print(f"mAP@0.5 = {out['mAP@0.5']:.4f}\nmAP@[0.5:0.95] = {out['mAP@[0.5:0.95]']:.4f}")
        print(f"mAP@0.3 = {out['mAP@0.3']:.4f}\nmAP@[0.3:0.7] = {out['mAP@[0.3:0.7]']:.4f}")
    return out
