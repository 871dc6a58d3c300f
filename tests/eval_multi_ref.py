"""NumPy restatement of the device evaluation (csrc/rtn_eval.hip through model/eval.py DeviceEvaluator): split_detections on
detect-format arrays, the greedy match at several IoU thresholds at once (each threshold its own set of taken annotations), AP per
class and threshold, P/R/F1 at a score threshold and the IoU-weighted F1.  AP comes from oracle/ref_eval.ap_from_hits, so at
t = 0.5 this agrees with oracle.ref_eval.evaluate_detections (tests/test_eval_device.py checks it)."""
import numpy as np

from oracle import ref_numpy as R
from oracle.ref_eval import ap_from_hits

COCO = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))


def split(boxes, scores, labels, num_classes, scale, score_threshold=0.05, max_detections=300):
    """One image's (D,4) / (D,) / (D,) detect outputs -> kept index list and per-class (n,5) arrays in original coordinates."""
    s = np.asarray(scores, np.float32).astype(np.float64)
    keep = np.flatnonzero(s > score_threshold)[:max_detections]
    lab = np.asarray(labels)[keep]
    b = np.asarray(boxes, np.float32).astype(np.float64)[keep] / scale
    per_class = [np.concatenate([b[lab == c], s[keep][lab == c, None]], 1) for c in range(num_classes)]
    return keep, lab, per_class


def match_image(dets, anns, thresholds):
    """dets (n,5) of one class (kept-index order), anns (m,4) -> hit mask per detection (bit t: hit at thresholds[t])."""
    n = dets.shape[0]
    masks = np.zeros(n, np.int64)
    if n == 0 or anns.shape[0] == 0:
        return masks
    order = np.argsort(-dets[:, 4], kind="stable")
    iou = R.compute_overlap(dets[order, :4], anns)
    taken = [set() for _ in thresholds]
    for rank, k in enumerate(order):
        j = int(np.argmax(iou[rank]))
        for t, thr in enumerate(thresholds):
            if iou[rank, j] >= np.float32(thr) and j not in taken[t]:      # float32 compare, as NumPy 2 does for f32 vs float
                taken[t].add(j)
                masks[k] |= 1 << t
    return masks


def evaluate(images, annotations, scales, num_classes, thresholds, score_threshold=0.05, max_detections=300, f1_score_threshold=0.5):
    """images: [(boxes (D,4), scores (D,), labels (D,))], annotations: [(m,5) original coordinates], scales: [float].
    Returns (summary dict with the keys of model/eval.py summarize(), slots) where slots[i] = (class, score, mask) per kept index
    (class -1 for a kept row whose label is outside the classes, and for the empty slots up to max_detections)."""
    T = len(thresholds)
    per_class = {c: [] for c in range(num_classes)}               # (score, mask) in image order, then per-class score order
    n_ann = np.zeros(num_classes, np.int64)
    slots = []
    for (boxes, scores, labels), ann, scale in zip(images, annotations, scales):
        keep, lab, dets = split(boxes, scores, labels, num_classes, scale, score_threshold, max_detections)
        ann = np.asarray(ann, np.float64).reshape(-1, 5)
        cls = np.full(max_detections, -1, np.int64)
        sc = np.zeros(max_detections, np.float32)
        mk = np.zeros(max_detections, np.int64)
        for c in range(num_classes):
            a = ann[ann[:, 4] == c, :4]
            n_ann[c] += a.shape[0]
            idx = np.flatnonzero(lab == c)
            m = match_image(dets[c], a, thresholds)
            cls[idx], sc[idx], mk[idx] = c, dets[c][:, 4].astype(np.float32), m
            order = np.argsort(-dets[c][:, 4], kind="stable")
            per_class[c] += [(dets[c][k, 4], m[k]) for k in order]
        slots.append((cls, sc, mk))
    ap, f1 = {}, {}
    for t, thr in enumerate(thresholds):
        ap[thr], f1[thr] = {}, {}
        for c in range(num_classes):
            s = np.array([v[0] for v in per_class[c]], np.float64)
            h = np.array([(v[1] >> t) & 1 for v in per_class[c]], bool)
            n = int(n_ann[c])
            ap[thr][c] = (ap_from_hits(s, h, n) if n else 0.0, n)
            above = s.astype(np.float32) >= np.float32(f1_score_threshold)
            TP = int(h[above].sum())
            FP = int(above.sum()) - TP
            FN = n - TP
            P = TP / (TP + FP) if TP + FP > 0 else 0.0
            Rc = TP / n if n > 0 else 0.0
            F = 2.0 * P * Rc / (P + Rc) if P + Rc > 0 else 0.0
            f1[thr][c] = (TP, FP, FN, P, Rc, F)
    mean = {}
    for thr in thresholds:
        present = [a for a, n in ap[thr].values() if n > 0]
        mean[thr] = float(sum(present) / len(present)) if present else 0.0
    micro = {}
    for thr in thresholds:
        TP, FP, FN = (sum(v[i] for v in f1[thr].values()) for i in range(3))
        P = TP / (TP + FP) if TP + FP > 0 else 0.0
        Rc = TP / (TP + FN) if TP + FN > 0 else 0.0
        micro[thr] = 2.0 * P * Rc / (P + Rc) if P + Rc > 0 else 0.0
    coco = all(c in thresholds for c in COCO)
    out = {"iou_thresholds": tuple(thresholds), "average_precision": ap, "f1": f1, "mean_ap": mean,
           "mAP": sum(mean.values()) / T, "map_50_95": float(np.mean([mean[c] for c in COCO])) if coco else None,
           "f1_micro": micro, "weighted_f1": sum(t * micro[t] for t in thresholds) / sum(thresholds)}
    return out, slots
