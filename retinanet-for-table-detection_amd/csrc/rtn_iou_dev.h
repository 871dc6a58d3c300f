// rtn_iou_dev.h — utils.compute_overlap (model/utils.py:180-211) for one (box, annotation) pair: f64 math, f32 result.
// Shared by rtn_compute_overlap (rtn_anchors.hip) and the evaluation match kernel (rtn_eval.hip), so both produce the same bits.
#pragma once
#include "rtn_internal.h"

__device__ __forceinline__ float rtn_iou_f64(const double* a, const double* b) {
#pragma clang fp contract(off)
    const double area1 = (a[2] - a[0]) * (a[3] - a[1]);
    const double area2 = (b[2] - b[0]) * (b[3] - b[1]);
    const double w = fmax(0.0, fmin(a[2], b[2]) - fmax(a[0], b[0]));
    const double hh = fmax(0.0, fmin(a[3], b[3]) - fmax(a[1], b[1]));
    const double inter = w * hh;
    return (float)(inter / (area1 + area2 - inter));
}
