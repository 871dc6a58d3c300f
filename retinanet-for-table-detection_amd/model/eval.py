"""Detection evaluator (AP at an IoU threshold) and the detection dump format — SURVEY §8(f) rank 1.

The reference has no evaluator (its training loop runs without validation: RetinaNet.py:149; test() only draws the
score-sorted boxes: RetinaNet.py:373-383), so there is nothing of the reference's to pin against: PARITY UNPINNED.  The
algorithm is the Pascal-VOC style evaluation published with keras-retinanet, the project the reference's model/ package
derives from:
  per class, over all images: detections sorted by descending score; a detection is a true positive when its best-IoU
  annotation (same image, same class) has IoU >= threshold and has not been matched before, otherwise a false positive;
  recall = cumTP / #annotations, precision = cumTP / (cumTP + cumFP); AP = area under the monotone precision envelope
  evaluated at every recall change (all-point interpolation).
IoU comes from the device (`rtn_compute_overlap`, the float32 IoU of model/utils.py:180-211): no GPU, no evaluator.

DeviceEvaluator / evaluate_generator run the same evaluation on the device (csrc/rtn_eval.hip) at up to 16 IoU thresholds at once,
with P/R/F1 at a score threshold, without a host sync per batch: callbacks.Evaluate uses them as a training metric.

validate_generator adds the validation loss to that pass: the forward that produces a batch's detections also feeds
rtn_retina_loss_boxes_fwd (focal + smooth-L1 per image, straight from the ground-truth boxes), so `val_loss` and mAP come from one
forward per group and one small copy at the end (customCallbacks.Validate).
"""
import copy
import csv
import ctypes as C

import numpy as np
import torch

from . import Parameters, _rt
from .utils import compute_overlap, compute_resize_scale


def compute_ap(recall, precision):
    """Area under the precision envelope; recall/precision are the cumulative curves in detection order."""
    mrec = np.concatenate(([0.], np.asarray(recall, np.float64), [1.]))
    mpre = np.concatenate(([0.], np.asarray(precision, np.float64), [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def evaluate_detections(all_detections, all_annotations, num_classes=1, iou_threshold=0.5):
    """all_detections[i][c]: (n,5) array [x1,y1,x2,y2,score] of image i, class c; all_annotations[i][c]: (m,4) boxes.
    Returns {class: (average_precision, num_annotations)}."""
    result = {}
    for label in range(num_classes):
        scores, hits = [], []
        num_annotations = 0
        for dets, anns in zip(all_detections, all_annotations):
            d = np.asarray(dets[label], np.float64).reshape(-1, 5)
            a = np.asarray(anns[label], np.float64).reshape(-1, 4)
            num_annotations += a.shape[0]
            if d.shape[0] == 0:
                continue
            order = np.argsort(-d[:, 4], kind="stable")
            d = d[order]
            taken = np.zeros(a.shape[0], dtype=bool)
            iou = compute_overlap(d[:, :4], a) if a.shape[0] else None        # one device call per image
            for k in range(d.shape[0]):
                scores.append(d[k, 4])
                if a.shape[0] == 0:
                    hits.append(False)
                    continue
                j = int(np.argmax(iou[k]))
                if iou[k, j] >= iou_threshold and not taken[j]:
                    taken[j] = True
                    hits.append(True)
                else:
                    hits.append(False)
        if num_annotations == 0:
            result[label] = (0.0, 0)
            continue
        order = np.argsort(-np.asarray(scores, np.float64), kind="stable")
        tp = np.cumsum(np.asarray(hits, bool)[order]).astype(np.float64)
        fp = np.cumsum(~np.asarray(hits, bool)[order]).astype(np.float64)
        recall = tp / num_annotations
        precision = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        result[label] = (compute_ap(recall, precision), num_annotations)
    return result


def mean_ap(result, weighted=False):
    """mAP over the classes that have annotations (optionally weighted by their annotation counts)."""
    present = [(ap, n) for ap, n in result.values() if n > 0]
    if not present:
        return 0.0
    if weighted:
        return float(sum(ap * n for ap, n in present) / sum(n for _, n in present))
    return float(sum(ap for ap, _ in present) / len(present))


def split_detections(boxes, scores, labels, num_classes=1, scale=1.0, score_threshold=0.05, max_detections=300):
    """One image's padded inference outputs ((300,4), (300,), (300,), -1 padded: model/defineModel.py:310-315) ->
    per-class (n,5) arrays in ORIGINAL image coordinates (boxes divided by the resize scale, RetinaNet.py:366-367)."""
    boxes, scores, labels = np.asarray(boxes, np.float64) / scale, np.asarray(scores, np.float64), np.asarray(labels)
    keep = np.where(scores > score_threshold)[0][:max_detections]
    out = []
    for c in range(num_classes):
        idx = keep[labels[keep] == c]
        out.append(np.concatenate([boxes[idx], scores[idx, None]], axis=1))
    return out


def write_detections_csv(path, image_ids, per_image_detections, class_names=None):
    """Detection dump: the reference's annotation CSV row (csv_generator.py:16-52: image_id,xmin,ymin,xmax,ymax,label)
    with the score appended."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        for image_id, dets in zip(image_ids, per_image_detections):
            for c, d in enumerate(dets):
                name = class_names[c] if class_names else c
                for x1, y1, x2, y2, s in np.asarray(d, np.float64).reshape(-1, 5):
                    w.writerow([image_id, "%.2f" % x1, "%.2f" % y1, "%.2f" % x2, "%.2f" % y2, name, "%.6f" % s])


def read_detections_csv(path, class_ids=None):
    """Inverse of write_detections_csv -> {image_id: {class: (n,5) array}}."""
    out = {}
    with open(path, newline="") as f:
        for image_id, x1, y1, x2, y2, label, score in csv.reader(f):
            c = class_ids[label] if class_ids else int(label)
            out.setdefault(image_id, {}).setdefault(c, []).append([float(x1), float(y1), float(x2), float(y2), float(score)])
    return {k: {c: np.asarray(v, np.float64) for c, v in d.items()} for k, d in out.items()}


def evaluate(model, images, annotations, scales=None, num_classes=1, iou_threshold=0.5, score_threshold=0.05, max_detections=300):
    """Run an inference model (model/defineModel.py:retinanet_bbox) over preprocessed images [(H,W,3) ...] and score it.
    annotations[i]: (m,5) [x1,y1,x2,y2,label] in original coordinates; scales[i]: resize scale of image i."""
    all_dets, all_anns = [], []
    for i, img in enumerate(images):
        boxes, scores, labels = model.predict_on_batch(np.expand_dims(img, 0))[:3]
        s = 1.0 if scales is None else scales[i]
        all_dets.append(split_detections(boxes[0], scores[0], labels[0], num_classes, s, score_threshold, max_detections))
        ann = np.asarray(annotations[i], np.float64).reshape(-1, 5)
        all_anns.append([ann[ann[:, 4] == c, :4] for c in range(num_classes)])
    return evaluate_detections(all_dets, all_anns, num_classes, iou_threshold)


COCO_IOU_THRESHOLDS = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))     # 0.50:0.05:0.95


def _micro_f1(tp, fp, fn):
    p = tp / (tp + fp) if tp + fp > 0 else 0.0
    r = tp / (tp + fn) if tp + fn > 0 else 0.0
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def summarize(iou_thresholds, average_precision, f1):
    """The result dict of DeviceEvaluator.result() (tests/eval_multi_ref.py builds the same one from its NumPy restatement):
      average_precision[t][c] = (AP, n_ann)                      evaluate_detections' {class: (AP, n_ann)} at IoU threshold t
      f1[t][c] = (TP, FP, FN, P, R, F1)                          at the score threshold f1_score_threshold
      mean_ap[t]                                                 mean_ap(average_precision[t]): classes with annotations
      mAP                                                        mean of mean_ap over the requested thresholds
      map_50_95                                                  the same over 0.50:0.05:0.95 when all ten were requested, else None
      f1_micro[t]                                                F1 of TP, FP, FN summed over the classes
      weighted_f1                                                sum_t t * f1_micro[t] / sum_t t (the IoU-weighted F1 of ICDAR cTDaR)"""
    ts = [float(t) for t in iou_thresholds]
    mean = {t: mean_ap(average_precision[t]) for t in ts}
    micro = {}
    for t in ts:
        tp, fp, fn = (sum(v[i] for v in f1[t].values()) for i in range(3))
        micro[t] = _micro_f1(tp, fp, fn)
    coco = all(any(abs(t - c) < 1e-9 for t in ts) for c in COCO_IOU_THRESHOLDS)
    return {"iou_thresholds": tuple(ts), "average_precision": average_precision, "f1": f1, "mean_ap": mean,
            "mAP": float(sum(mean.values()) / len(ts)),
            "map_50_95": float(np.mean([mean[t] for t in ts if any(abs(t - c) < 1e-9 for c in COCO_IOU_THRESHOLDS)])) if coco else None,
            "f1_micro": micro, "weighted_f1": float(sum(t * micro[t] for t in ts) / sum(ts))}


class DeviceEvaluator:
    """evaluate_detections (+ split_detections) on the device, for up to 16 IoU thresholds at once (csrc/rtn_eval.hip).

    add() takes one batch exactly as Engine.detect returns it - boxes (B,D,4) at network scale, scores (B,D), labels (B,D), device
    tensors (NumPy arrays are uploaded) - with each image's resize scale and its annotations in ORIGINAL coordinates ((m,5) arrays
    [x1,y1,x2,y2,label], or {'bboxes', 'labels'} dicts as Generator.load_annotations returns them).  It enqueues the match on
    `stream` (default: the current stream) - the stream that produced the detections - and returns without a host sync.
    result() runs the finalize kernels on the current stream and makes one small device-to-host copy: see summarize()."""

    def __init__(self, num_classes, iou_thresholds=(0.5,), score_threshold=0.05, max_detections=300, f1_score_threshold=0.5,
                 device=None):
        self.K = int(num_classes)
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        self.T = len(self.iou_thresholds)
        if not 1 <= self.T <= 16:
            raise ValueError("1 to 16 IoU thresholds, got %d" % self.T)
        if not all(0.0 < t <= 1.0 for t in self.iou_thresholds):
            raise ValueError("IoU thresholds must be in (0, 1], got %s" % (self.iou_thresholds,))
        if not (score_threshold >= 0.0):
            raise ValueError("score_threshold must be >= 0 (the device sort orders the score bits), got %r" % score_threshold)
        if not 1 <= int(max_detections) <= _rt.L.RTN_MAX_DET:
            raise ValueError("max_detections must be in [1, %d]" % _rt.L.RTN_MAX_DET)
        if not 1 <= self.K <= 65535:
            raise ValueError("num_classes must be in [1, 65535]")
        self.score_threshold, self.S, self.f1_score_threshold = float(score_threshold), int(max_detections), float(f1_score_threshold)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._h = _rt.L.Handle(self.device.index)
        self._thr = (C.c_double * self.T)(*self.iou_thresholds)
        self.counts = torch.zeros(2 * self.K, dtype=torch.int32, device=self.device)
        self.slots = torch.empty(0, 2, dtype=torch.int32, device=self.device)
        self.num_images = 0
        self._events = []               # matches enqueued on streams other than the caller's: result() waits for them
        self._ws = None

    def _join(self):
        cur = torch.cuda.current_stream(self.device)
        for ev in self._events:
            cur.wait_event(ev)
        self._events = []

    def reserve(self, num_images):
        """Room for `num_images` images in all.  The host decides (it knows the image count without asking the device); growing
        copies the slots written so far on the current stream, after every match enqueued elsewhere."""
        need = int(num_images) * self.S
        if need <= self.slots.shape[0]:
            return
        self._join()
        grown = torch.empty(max(need, 2 * self.slots.shape[0]), 2, dtype=torch.int32, device=self.device)
        if self.num_images:
            grown[:self.num_images * self.S].copy_(self.slots[:self.num_images * self.S])
        self.slots = grown

    def _annotations(self, annotations):
        B = len(annotations)
        gb = np.zeros((B, _rt.L.RTN_MAX_GT, 4), np.float64)
        gl = np.zeros((B, _rt.L.RTN_MAX_GT), np.int32)
        gc = np.zeros((B,), np.int32)
        for i, a in enumerate(annotations):
            if isinstance(a, dict):
                boxes, labels = np.asarray(a["bboxes"], np.float64).reshape(-1, 4), np.asarray(a["labels"]).reshape(-1)
            else:
                a = np.asarray(a, np.float64).reshape(-1, 5)
                boxes, labels = a[:, :4], a[:, 4]
            n = boxes.shape[0]
            if n > _rt.L.RTN_MAX_GT:
                raise ValueError("at most %d annotations per image are supported, got %d" % (_rt.L.RTN_MAX_GT, n))
            gb[i, :n], gl[i, :n], gc[i] = boxes, labels.astype(np.int32), n
        return gb, gl, gc

    def add(self, boxes, scores, labels, scales, annotations, stream=None):
        B, D = int(scores.shape[0]), int(scores.shape[1])
        if tuple(boxes.shape) != (B, D, 4) or tuple(labels.shape) != (B, D):
            raise ValueError("boxes (B,D,4), scores (B,D), labels (B,D) expected, got %s %s %s"
                             % (tuple(boxes.shape), tuple(scores.shape), tuple(labels.shape)))
        if len(annotations) != B or len(scales) != B:
            raise ValueError("one scale and one annotation set per image: %d images, %d scales, %d annotation sets"
                             % (B, len(scales), len(annotations)))
        if B == 0:
            return
        host = self._annotations(annotations) + (np.asarray(scales, np.float64).reshape(B),)
        self.reserve(self.num_images + B)
        caller = torch.cuda.current_stream(self.device)
        st = stream if stream is not None else caller
        with torch.cuda.stream(st):
            gb, gl, gc, sc = [torch.from_numpy(a).pin_memory().to(self.device, non_blocking=True) for a in host]
            b = _rt.dev(boxes, torch.float32)
            s = _rt.dev(scores, torch.float32)
            lab = _rt.dev(labels, torch.int32)
            self._h.set_stream(st.cuda_stream)
            first = self.slots[self.num_images * self.S:]
            self._h.check(_rt.L.lib.rtn_eval_match(self._h.raw, B, D, b.data_ptr(), s.data_ptr(), lab.data_ptr(), sc.data_ptr(),
                                                   gb.data_ptr(), gl.data_ptr(), gc.data_ptr(), _rt.L.RTN_MAX_GT, self.K, self.T,
                                                   self._thr, self.score_threshold, self.S, first.data_ptr(), self.counts.data_ptr()))
            if st != caller:
                ev = torch.cuda.Event()
                ev.record(st)
                self._events.append(ev)
        self.num_images += B

    def result(self, extra=None):
        """extra: a float64 device tensor that rides in the same device-to-host copy (validate_generator's per-image loss sums);
        with it the return value is (result, extra on the host as a NumPy array of extra's shape)."""
        K, T = self.K, self.T
        extra_host = None
        ap = {t: {c: (0.0, 0) for c in range(K)} for t in self.iou_thresholds}
        f1 = {t: {c: (0, 0, 0, 0.0, 0.0, 0.0) for c in range(K)} for t in self.iou_thresholds}
        if self.num_images:
            self._join()
            nb = int(_rt.L.lib.rtn_eval_workspace_bytes(self.num_images * self.S, K, T))
            if nb <= 0:
                raise ValueError("rtn_eval_workspace_bytes: unsupported shape (%d images)" % self.num_images)
            if self._ws is None or self._ws.numel() < nb:
                self._ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
            out = torch.empty(K * T * 8, dtype=torch.float64, device=self.device)
            self._h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
            self._h.check(_rt.L.lib.rtn_eval_finalize(self._h.raw, self.num_images, self.S, self.slots.data_ptr(), self.counts.data_ptr(),
                                                      K, T, self.f1_score_threshold, out.data_ptr(), self._ws.data_ptr(),
                                                      self._ws.numel()))
            if extra is not None:
                both = torch.cat([out, extra.reshape(-1)]).cpu().numpy()
                r, extra_host = both[:K * T * 8].reshape(K, T, 8), both[K * T * 8:].reshape(tuple(extra.shape))
            else:
                r = out.cpu().numpy().reshape(K, T, 8)
            for ti, t in enumerate(self.iou_thresholds):
                for c in range(K):
                    v = r[c, ti]
                    ap[t][c] = (float(v[0]), int(v[1]))
                    f1[t][c] = (int(v[2]), int(v[3]), int(v[4]), float(v[5]), float(v[6]), float(v[7]))
        if extra is not None:
            return summarize(self.iou_thresholds, ap, f1), (extra_host if extra_host is not None else extra.cpu().numpy())
        return summarize(self.iou_thresholds, ap, f1)

    def slot_view(self):
        """(score f32, hit mask, class) of every slot [image][kept index] (class -1: empty): the match stage's output, for tests."""
        torch.cuda.synchronize(self.device)
        self._events = []
        raw = self.slots[:self.num_images * self.S].cpu().numpy().view(np.uint32).reshape(self.num_images, self.S, 2)
        empty = raw[..., 1] == 0xFFFFFFFF
        cls = np.where(empty, -1, (raw[..., 1] >> 16).astype(np.int64))
        mask = np.where(empty, 0, (raw[..., 1] & 0xFFFF).astype(np.int64))
        return raw[..., 0].view(np.float32), mask, cls


def _load_batch(generator, group):
    """The pages of `group` (device, uint8) and their canvas, built by the generator's own compute_inputs on its stream without
    augmentation; the canvas is handed over to the current stream.  Returns (canvas, scales, annotations as loaded, pages)."""
    images = generator.load_image_group(group)
    annotations = generator.load_annotations_group(group)
    with generator._lock, torch.cuda.stream(generator._stream):
        generator._h.set_stream(generator._stream.cuda_stream)
        pages = [generator._upload(im) for im in images]
        scales = [compute_resize_scale(p.shape, generator.image_min_side, generator.image_max_side) for p in pages]
        canvas, _ = generator.compute_inputs(pages, scales)
        done = torch.cuda.Event()
        done.record(generator._stream)
    cur = torch.cuda.current_stream(generator.device)
    cur.wait_event(done)
    canvas.record_stream(cur)
    return canvas, scales, annotations, pages


def _generator_batch(generator, group):
    """The inputs half of Generator.compute_input_output (csv_generator.py:373-398) without augmentation: the pages of `group`
    resized into one canvas by the generator's own compute_inputs on its stream, their resize scales, and their annotations in
    original coordinates (load_annotations_group).  Returns (canvas on the current stream's order, scales, annotations)."""
    return _load_batch(generator, group)[:3]


def evaluate_generator(model, generator, iou_thresholds=(0.5,), score_threshold=0.05, max_detections=300, f1_score_threshold=0.5,
                       in_flight=2, steps=None):
    """Evaluate an inference model (retinanet_bbox) on the groups of a CSVGenerator-style generator, all on the device: its pages go
    through the generator's own load_image_group / compute_inputs (the canvases it builds for training, without augmentation) and
    Engine.detect with `in_flight` batches at a time, as in Model.predict_generator; each batch's detections are matched on the
    stream that produced them (DeviceEvaluator.add) and nothing is read back until the one small copy of the result.
    Returns DeviceEvaluator.result()."""
    if not getattr(model, "bbox", False):
        raise ValueError("evaluate_generator: the inference model (retinanet_bbox / convert_model) is needed")
    eng = model.engine()
    modes = {"nms": model.nms, "class_specific_filter": model.class_specific_filter}
    groups = generator.groups if steps is None else generator.groups[:int(steps)]
    ev = DeviceEvaluator(model.num_classes, iou_thresholds, score_threshold, max_detections, f1_score_threshold,
                         device=eng.device.index)
    ev.reserve(sum(len(g) for g in groups))
    prev = eng.in_flight
    eng.join()
    eng.in_flight = max(1, int(in_flight))
    try:
        for group in groups:
            canvas, scales, annotations = _generator_batch(generator, group)
            x = _rt.dev(canvas, torch.float32)
            boxes, scores, labels = eng.detect(x, **modes)          # the model's own FilterDetections, as predict_on_batch
            st = eng.slot_stream(eng.last_slot) if eng.in_flight > 1 and not eng.training else None
            ev.add(boxes, scores, labels, scales, annotations, stream=st)
    finally:
        eng.join()
        eng.in_flight = prev
    return ev.result()


def _loss_annotations(generator, group, annotations, pages, scales):
    """What compute_input_output (csv_generator.py:373-398) hands compute_targets for `group`, without augmentation: the
    generator's filter_annotations on (a copy of) the loaded annotations, boxes times the resize scale in float64, and each
    page's own resized (h, w) - in rtn_anchor_targets' layout, on the host."""
    _, annotations = generator.filter_annotations(pages, [copy.deepcopy(a) for a in annotations], group)
    B = len(group)
    gb = np.zeros((B, _rt.L.RTN_MAX_GT, 4), np.float64)
    gl = np.zeros((B, _rt.L.RTN_MAX_GT), np.int32)
    gc = np.zeros((B,), np.int32)
    hw = np.zeros((B, 2), np.int32)
    for i, (ann, p, s) in enumerate(zip(annotations, pages, scales)):
        boxes = np.asarray(ann['bboxes'], np.float64).reshape(-1, 4) * s
        n = boxes.shape[0]
        if n > _rt.L.RTN_MAX_GT:
            raise ValueError("at most %d ground-truth boxes per image are supported, got %d" % (_rt.L.RTN_MAX_GT, n))
        gb[i, :n], gl[i, :n], gc[i] = boxes, np.asarray(ann['labels']).astype(np.int32), n
        hw[i] = (int(np.rint(p.shape[0] * s)), int(np.rint(p.shape[1] * s)))
    return gb, gl, gc, hw


def combine_losses(image_sums, group_sizes):
    """Keras' rule for evaluate_generator on per-image sums (n, 4) = {focal, smooth-L1, positives, positives}: per group the
    loss is sum of the image sums / max(1, sum of positives) (model/losses.py:42,88 on the group's batch), a float32 as the loss
    tensor and the functors of model/losses.py yield it; across groups the mean weighted by group size
    (keras/engine/training_generator.py evaluate_generator: np.average(outs, weights=batch_sizes)), float64 on the host.
    Returns (classification_loss, regression_loss, loss)."""
    s = np.asarray(image_sums, np.float64).reshape(-1, 4)
    cls = reg = 0.0
    lo = 0
    for n in group_sizes:
        g = s[lo:lo + n].sum(axis=0)
        cls += n * float(np.float32(g[0] / max(1.0, g[2])))
        reg += n * float(np.float32(g[1] / max(1.0, g[3])))
        lo += n
    total = float(max(1, sum(group_sizes)))
    cls, reg = float(cls / total), float(reg / total)
    return cls, reg, cls + reg


def validate_generator(model, generator, iou_thresholds=(0.5,), score_threshold=0.05, max_detections=300, f1_score_threshold=0.5,
                       in_flight=2, steps=None, alpha=0.25, gamma=2.0, sigma=3.0):
    """evaluate_generator and the validation loss in ONE pass over the generator's groups: every group runs one forward
    (Engine.detect with `in_flight` batches at a time); on the stream that ran it the detections are matched (DeviceEvaluator.add,
    with what evaluate_generator gives it) and rtn_retina_loss_boxes_fwd computes each page's focal and smooth-L1 sums from the
    page's filtered annotations times its resize scale and its own resized (h, w) - what compute_input_output hands
    compute_targets - against the anchors of the model's plan.  No dense target tensor exists and nothing is read back per batch.
    Returns DeviceEvaluator.result() plus
      classification_loss, regression_loss, loss : combine_losses (the `val_*` numbers Keras' evaluate_generator reports)
      image_losses : (n, 4) float64 rows (image index, focal sum, smooth-L1 sum, positives), one per page in group order."""
    if not getattr(model, "bbox", False):
        raise ValueError("validate_generator: the inference model (retinanet_bbox / convert_model) is needed")
    eng = model.engine()
    modes = {"nms": model.nms, "class_specific_filter": model.class_specific_filter}
    groups = generator.groups if steps is None else generator.groups[:int(steps)]
    total = sum(len(g) for g in groups)
    ev = DeviceEvaluator(model.num_classes, iou_thresholds, score_threshold, max_detections, f1_score_threshold,
                         device=eng.device.index)
    ev.reserve(total)
    sums = torch.zeros(max(1, total), 4, dtype=torch.float64, device=eng.device)
    prev = eng.in_flight
    eng.join()
    eng.in_flight = max(1, int(in_flight))
    row = 0
    try:
        for group in groups:
            canvas, scales, annotations, pages = _load_batch(generator, group)
            host = _loss_annotations(generator, group, annotations, pages, scales)
            x = _rt.dev(canvas, torch.float32)
            gt = [torch.from_numpy(a).pin_memory().to(eng.device, non_blocking=True) for a in host]
            job = _rt.engine.BoxLoss(gt[0], gt[1], gt[2], gt[3], sums, row, alpha=alpha, gamma=gamma, sigma=sigma,
                                     negative_overlap=Parameters.negative_overlap, positive_overlap=Parameters.positive_overlap)
            boxes, scores, labels = eng.detect(x, loss=job, **modes)
            st = eng.slot_stream(eng.last_slot) if eng.in_flight > 1 and not eng.training else None
            ev.add(boxes, scores, labels, scales, annotations, stream=st)
            row += len(group)
    finally:
        eng.join()
        eng.in_flight = prev
    result, s = ev.result(extra=sums[:total])                 # the pass's one small copy: the evaluator's numbers and the sums
    cls, reg, loss = combine_losses(s, [len(g) for g in groups])
    index = np.asarray([i for g in groups for i in g], np.float64).reshape(-1, 1)
    result.update({"classification_loss": cls, "regression_loss": reg, "loss": loss,
                   "image_losses": np.concatenate([index, s[:, :3]], axis=1) if total else np.zeros((0, 4))})
    return result
