"""NumPy restatement of the reference's filter_detections (model/layers.py:177-264) in all four modes
(class_specific_filter x nms), for ONE image, built from the oracle's pieces (oracle.ref_numpy.nms_tf).

Returns boxes (max_det,4), scores (max_det,), labels (max_det,) i32 and the anchor index of every detection (max_det,) i64,
all padded with -1 (model/layers.py:248-253)."""
import numpy as np

from oracle import ref_numpy as R

F32 = np.float32


def filter_detections_modes(boxes, classification, class_specific_filter=True, nms=True, score_threshold=0.05, max_detections=300,
                            nms_threshold=0.5):
    boxes = np.asarray(boxes, dtype=F32)
    cls = np.asarray(classification, dtype=F32)
    N, K = cls.shape

    def _filter(scores, labels):                                          # :200-219
        idx = np.nonzero(scores > F32(score_threshold))[0]                # :202 (strict)
        if nms:                                                           # :204-214
            keep = R.nms_tf(boxes[idx], scores[idx], max_detections, nms_threshold)
            idx = idx[keep]
        return idx, labels[idx]                                           # :217-218

    if class_specific_filter:                                             # :221-229: per class, concatenated class-major
        parts = [_filter(cls[:, c], np.full(N, c, dtype=np.int64)) for c in range(K)]
        rows = np.concatenate([p[0] for p in parts]).astype(np.int64)
        labs = np.concatenate([p[1] for p in parts]).astype(np.int64)
    else:                                                                 # :230-233: best class per anchor
        rows, labs = _filter(cls.max(axis=1), cls.argmax(axis=1).astype(np.int64))   # argmax: first (lowest) class on ties
        rows = rows.astype(np.int64)
    sc = cls[rows, labs]                                                  # :236
    k = min(max_detections, len(sc))                                      # :238 tf.nn.top_k
    top = np.lexsort((np.arange(len(sc)), -sc.astype(np.float64)))[:k]   # ties -> lower position of the concatenation
    out_b = np.full((max_detections, 4), -1, dtype=F32)                   # :248-253
    out_s = np.full((max_detections,), -1, dtype=F32)
    out_l = np.full((max_detections,), -1, dtype=np.int32)
    out_i = np.full((max_detections,), -1, dtype=np.int64)
    out_b[:k] = boxes[rows[top]]
    out_s[:k] = sc[top]
    out_l[:k] = labs[top]
    out_i[:k] = rows[top]
    return out_b, out_s, out_l, out_i


def gather_other(other, indices):
    """other_ (model/layers.py:245,254): rows of `other` (N, ...) at the detections' indices, -1 where the index is -1."""
    other = np.asarray(other)
    out = np.full((len(indices),) + other.shape[1:], -1, dtype=other.dtype)
    ok = indices >= 0
    out[ok] = other[indices[ok]]
    return out
