// rtn_assign_dev.h — one anchor against one image's ground-truth boxes: the assignment body shared by
// anchor_targets_kernel (rtn_anchors.hip, writes the dense targets) and loss_boxes_kernel (rtn_loss.hip, feeds the loss terms
// without ever writing them).  Restates compute_gt_annotations (model/anchors.py:96-117), bbox_transform (:282-313) and the
// outside-the-image rule of anchor_targets_bbox (:85-90).
// Include AFTER the includer's `#pragma clang fp contract(off)`: the reference rounds every product and sum, and both includers
// compile this text under that setting.
#pragma once
#include "rtn_internal.h"
#include "rtn_anchor_dev.h"

// anchors_for_shape, f64: base + ((i + 0.5) * stride)
__device__ __forceinline__ void anchor_f64(const DevAnchorCfg& c, int n, double a[4]) {
    const AnchorIdx ai = locate(c, n);
    const double sx = ((double)ai.x + 0.5) * (double)c.stride[ai.level];
    const double sy = ((double)ai.y + 0.5) * (double)c.stride[ai.level];
    const double* b = c.base[ai.level][ai.a];
    a[0] = b[0] + sx; a[1] = b[1] + sy; a[2] = b[2] + sx; a[3] = b[3] + sy;
}

// One image's boxes in shared memory.  gt_count is clamped to [0, RTN_MAX_GT]; ends with a barrier.  Returns the clamped count.
struct GtShared {
    double box[RTN_MAX_GT][4];
    double area[RTN_MAX_GT];
    int lab[RTN_MAX_GT];
};

__device__ __forceinline__ int stage_gt(GtShared& s, int b, const double* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                        const int* __restrict__ gt_count) {
    int G = gt_count[b];
    G = G < 0 ? 0 : (G > RTN_MAX_GT ? RTN_MAX_GT : G);
    for (int i = threadIdx.x; i < G; i += blockDim.x) {
        const double* g = gt_boxes + ((long long)b * RTN_MAX_GT + i) * 4;
        s.box[i][0] = g[0]; s.box[i][1] = g[1]; s.box[i][2] = g[2]; s.box[i][3] = g[3];
        s.area[i] = (g[2] - g[0]) * (g[3] - g[1]);
        s.lab[i] = gt_labels[(long long)b * RTN_MAX_GT + i];
    }
    __syncthreads();
    return G;
}

struct AnchorTarget {
    float state;    // 1 positive, 0 negative, -1 ignored
    float t[4];     // box deltas against the argmax box, rounded to float32 (zeros without boxes)
    int label;      // class of the argmax box for a positive anchor, else -1
};

__device__ __forceinline__ AnchorTarget assign_anchor(const double a[4], const GtShared& s, int G, float neg_ov, float pos_ov,
                                                      int img_h, int img_w) {
    AnchorTarget r;
    r.state = 0.f;
    r.t[0] = 0.f; r.t[1] = 0.f; r.t[2] = 0.f; r.t[3] = 0.f;
    r.label = -1;
    if (G > 0) {
        const double area1 = (a[2] - a[0]) * (a[3] - a[1]);
        float best = 0.f;
        int arg = 0;
        for (int i = 0; i < G; ++i) {
            const double x1 = fmax(a[0], s.box[i][0]);
            const double y1 = fmax(a[1], s.box[i][1]);
            const double x2 = fmin(a[2], s.box[i][2]);
            const double y2 = fmin(a[3], s.box[i][3]);
            const double w = fmax(0.0, x2 - x1);
            const double hh = fmax(0.0, y2 - y1);
            const double inter = w * hh;
            const double uni = area1 + s.area[i] - inter;
            const float iou = (float)(inter / uni);          // result array is float32
            if (i == 0 || iou > best) { best = iou; arg = i; }  // np.argmax: first maximum
        }
        const bool positive = best >= pos_ov;
        const bool ignore = (best > neg_ov) && !positive;
        r.state = positive ? 1.f : (ignore ? -1.f : 0.f);
        if (positive) r.label = s.lab[arg];
        // bbox_transform over ALL anchors with their argmax box
        const double aw = a[2] - a[0], ah = a[3] - a[1];
        r.t[0] = (float)(((s.box[arg][0] - a[0]) / aw) / 0.2);
        r.t[1] = (float)(((s.box[arg][1] - a[1]) / ah) / 0.2);
        r.t[2] = (float)(((s.box[arg][2] - a[2]) / aw) / 0.2);
        r.t[3] = (float)(((s.box[arg][3] - a[3]) / ah) / 0.2);
    }
    // anchors whose centre lies outside this image's own extent are ignored
    const double cx = (a[0] + a[2]) / 2, cy = (a[1] + a[3]) / 2;
    if (cx >= (double)img_w || cy >= (double)img_h) r.state = -1.f;
    return r;
}
