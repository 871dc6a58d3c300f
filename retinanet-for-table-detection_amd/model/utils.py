"""model/utils.py of the reference: image utilities (:19-211) and model utilities (:218-259) on the device."""
import sys
import warnings

import numpy as np
import torch

from . import _pages, _rt
from .Parameters import image_scaling_factor, image_subtraction_factor
from .page_io import write_image, write_images_bgr, encode_jpeg_bgr, encode_png_bgr, decode_png_bgr, decode_tiff_bgr, encode_tiff_bgr, JPEG_EXTENSIONS  # noqa: F401

L = _rt.L


def preprocess_image(x, mode='tf'):
    """ model/utils.py:19-47: float32 cast, then 'tf' x/127.5-1 | 'caffe' BGR mean subtraction | 'custom_tf' x/127.5-1."""
    x = np.asarray(x)
    code = {'tf': 0, 'caffe': 1, 'custom_tf': 2}.get(mode)
    if code is None:
        return x.astype(np.float32)
    h = _rt.handle()
    src = _rt.dev(x, torch.uint8 if x.dtype == np.uint8 else torch.float32)
    out = torch.empty(src.shape, dtype=torch.float32, device="cuda")
    h.check(L.lib.rtn_preprocess_image(h.raw, src.data_ptr(), 2 if x.dtype == np.uint8 else 1, out.data_ptr(), src.numel(), code,
                                       float(image_scaling_factor), float(image_subtraction_factor)))
    return _rt.host(out)


def shift(shape, stride, anchors):
    """ model/utils.py:51-80 (the in-graph float32 twin of anchors.shift): anchors shifted over a (rows, cols) map,
    centres (i + 0.5) * stride, order y -> x -> anchor -> (shape[0] * shape[1] * A, 4) float32 (rtn_anchors_f32)."""
    import ctypes as C
    from . import anchors as _anchors
    base = np.asarray(anchors, np.float32)
    h = _rt.handle()
    cfg, n = _anchors._cfg([shape], [stride], [base.astype(np.float64)])
    out = torch.empty(n, 4, dtype=torch.float32, device="cuda")
    h.check(L.lib.rtn_anchors_f32(h.raw, C.byref(cfg), out.data_ptr()))
    return _rt.host(out)


def bbox_transform_inv(boxes, deltas, mean=None, std=None):
    """ model/utils.py:84-112: boxes (B, N, 4) + deltas * std + mean applied to the box width / height (rtn_regress_boxes,
    the kernel behind layers.RegressBoxes)."""
    import ctypes as C
    if mean is None:
        mean = [0, 0, 0, 0]
    if std is None:
        std = [0.2, 0.2, 0.2, 0.2]
    h = _rt.handle()
    a, r = _rt.dev(np.asarray(boxes), torch.float32), _rt.dev(np.asarray(deltas), torch.float32)
    if a.shape != r.shape or a.shape[-1] != 4:
        raise ValueError("boxes and deltas must both be (B, N, 4), got %s and %s" % (tuple(a.shape), tuple(r.shape)))
    out = torch.empty_like(a)
    m4 = (C.c_float * 4)(*[float(v) for v in mean])
    s4 = (C.c_float * 4)(*[float(v) for v in std])
    h.check(L.lib.rtn_regress_boxes(h.raw, a.data_ptr(), r.data_ptr(), a.numel() // 4, m4, s4, out.data_ptr()))
    return _rt.host(out)


def compute_resize_scale(image_shape, min_side=800, max_side=1333):
    """ model/utils.py:116-137."""
    (rows, cols, _) = image_shape
    smallest_side = min(rows, cols)
    scale = min_side / smallest_side
    largest_side = max(rows, cols)
    if largest_side * scale > max_side:
        scale = max_side / largest_side
    return scale


def resize_image(img, min_side=800, max_side=1333):
    """ model/utils.py:140-154: bicubic (cv2.INTER_CUBIC) resize by the computed scale. Returns (image, scale)."""
    from . import preprocess
    scale = compute_resize_scale(img.shape, min_side=min_side, max_side=max_side)
    return preprocess.resize_cubic(img, scale), scale


def _compute_overlap_device(boxes1, boxes2):
    h = _rt.handle()
    a, b = _rt.dev(np.asarray(boxes1, np.float64), torch.float64), _rt.dev(np.asarray(boxes2, np.float64), torch.float64)
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device="cuda")
    h.check(L.lib.rtn_compute_overlap(h.raw, a.data_ptr(), b.data_ptr(), a.shape[0], b.shape[0], out.data_ptr()))
    return out


def compute_overlap(boxes1, boxes2):
    """ model/utils.py:180-211 -> (len(boxes1), len(boxes2)) float32 IoU."""
    if len(boxes1) == 0 or len(boxes2) == 0:
        return np.zeros((len(boxes1), len(boxes2)), dtype=np.float32)
    return _rt.host(_compute_overlap_device(boxes1, boxes2))


def convert_model(model, nms=True, class_specific_filter=True, anchor_params=None):
    """ model/utils.py:218-231: training model -> inference model.  Unlike the reference, `nms` takes effect: the reference
    passes it as retinanet_bbox(nms=...), which has no such parameter and drops it into **kwargs, so its
    converted models always run NMS.  Here it is retinanet_bbox's applyNms."""
    from .defineModel import retinanet_bbox
    return retinanet_bbox(model=model, applyNms=nms, class_specific_filter=class_specific_filter, anchor_params=anchor_params)


def assert_training_model(model):
    """ model/utils.py:234-238."""
    assert(all(output in model.output_names for output in ['regression', 'classification'])), \
        "Input is not a training model (no 'regression' and 'classification' outputs were found, outputs are: {}).".format(model.output_names)


def check_training_model(model):
    """ model/utils.py:241-248."""
    try:
        assert_training_model(model)
    except AssertionError as e:
        print(e, file=sys.stderr)
        sys.exit(1)


def freeze(model):
    """ model/utils.py:251-259."""
    for layer in model.layers:
        layer.trainable = False
    return model


# ---- visualisation utilities (model/utils.py:267-373) and the per-page output step of RetinaNet.py:348-402 -----------------------
# Host-side raster work on the ORIGINAL page for a handful of boxes: NumPy + Pillow in place of cv2.
# Pixel parity with OpenCV's anti-aliased rectangle and Hershey text is not claimed (parity unpinned; SampleResults/*.png in the
# reference are qualitative); box geometry, colours, crop extents and output file names follow the reference.
def label_color(label):
    """ model/utils.py:267-283: colour `label` of 80 evenly spaced fully saturated hues, as a list of three ints."""
    import warnings
    if 0 <= label < 80:
        h = (label * (1.0 / 80)) * 6.0                     # np.arange(0, 1, 1/80)[label], then matplotlib's hsv_to_rgb at s = v = 1
        i, f = int(h) % 6, h - int(h)
        q, t = 1.0 - f, 1.0 - (1.0 - f)
        r, g, b = [(1, t, 0), (q, 1, 0), (0, 1, t), (0, q, 1), (t, 0, 1), (1, 0, q)][i]
        return [int(255 * r), int(255 * g), int(255 * b)]
    warnings.warn('Label {} has no color, returning default.'.format(label))
    return 0, 255, 0


def extract_box(image, box):
    """ model/utils.py:286-295: the sub-image image[y1:y2, x1:x2]."""
    b = np.array(box).astype(int)
    return image[b[1]:b[3], b[0]:b[2]]


def draw_box(image, box, color, thickness=5):
    """ model/utils.py:297-307.  The reference hands cv2.rectangle the colour 0 whatever `color` is (:307), so its boxes are black;
    kept.  The outline is centred on the box edges and `thickness` pixels wide, clipped to the image, drawn in place."""
    b = np.array(box).astype(int)
    H, W = image.shape[:2]
    lo, hi = thickness // 2, thickness - thickness // 2
    x1, y1, x2, y2 = min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])

    def band(ya, yb, xa, xb):
        ya, yb, xa, xb = max(ya, 0), min(yb, H), max(xa, 0), min(xb, W)
        if ya < yb and xa < xb:
            image[ya:yb, xa:xb] = 0

    band(y1 - lo, y1 + hi, x1 - lo, x2 + hi)
    band(y2 - lo, y2 + hi, x1 - lo, x2 + hi)
    band(y1 - lo, y2 + hi, x1 - lo, x1 + hi)
    band(y1 - lo, y2 + hi, x2 - lo, x2 + hi)


def _caption_mask(caption, font_size=5):
    """The pixels draw_caption paints for `caption`, as a bool (h, w) mask whose top-left pixel goes to (x1, y1 - 10 - h): Pillow's
    built-in font, every font pixel blown up to a square of round(0.9 font_size) pixels."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default()
    probe = ImageDraw.Draw(Image.new("L", (1, 1)))
    l, t, r, btm = probe.textbbox((0, 0), caption, font=font)
    tile = Image.new("L", (max(r, 1), max(btm, 1)), 0)
    ImageDraw.Draw(tile).text((0, 0), caption, fill=255, font=font)
    s = max(1, int(round(font_size * 0.9)))
    return np.kron(np.asarray(tile) > 127, np.ones((s, s), bool))


def draw_caption(image, box, caption, font_size=5, font_thickness=5):
    """ model/utils.py:310-318: `caption` above the box's top-left corner in (0, 0, 255), drawn in place (Pillow's built-in font
    scaled by font_size in place of FONT_HERSHEY_PLAIN)."""
    b = np.array(box).astype(int)
    mask = _caption_mask(caption, font_size)
    x0, y0 = int(b[0]), int(b[1]) - 10 - mask.shape[0]
    H, W = image.shape[:2]
    ys, xs = max(y0, 0), max(x0, 0)
    ye, xe = min(y0 + mask.shape[0], H), min(x0 + mask.shape[1], W)
    if ys < ye and xs < xe:
        m = mask[ys - y0:ye - y0, xs - x0:xe - x0]
        region = image[ys:ye, xs:xe]
        region[m] = (0, 0, 255) if image.ndim == 3 else 255


def draw_boxes(image, boxes, color, thickness=2):
    """ model/utils.py:321-330."""
    for b in boxes:
        draw_box(image, b, color, thickness=thickness)


def draw_detections(image, boxes, scores, labels, color=None, label_to_name=None, score_threshold=0.5):
    """ model/utils.py:333-352."""
    for i in np.where(scores > score_threshold)[0]:
        c = color if color is not None else label_color(labels[i])
        draw_box(image, boxes[i, :], color=c)
        caption = str(label_to_name(labels[i]) if label_to_name else labels[i]) + ': {0:.2f}'.format(scores[i])
        draw_caption(image, boxes[i, :], caption)


def draw_annotations(image, annotations, color=(0, 255, 0), label_to_name=None):
    """ model/utils.py:355-373."""
    if isinstance(annotations, np.ndarray):
        annotations = {'bboxes': annotations[:, :4], 'labels': annotations[:, 4]}
    assert('bboxes' in annotations)
    assert('labels' in annotations)
    assert(annotations['bboxes'].shape[0] == annotations['labels'].shape[0])
    for i in range(annotations['bboxes'].shape[0]):
        label = annotations['labels'][i]
        c = color if color is not None else label_color(label)
        draw_caption(image, annotations['bboxes'][i], '{}'.format(label_to_name(label) if label_to_name else label))
        draw_box(image, annotations['bboxes'][i], color=c)


def _kept_detections(boxes, scores, labels, image_scale, score_threshold):
    """The detections render_detections keeps of one page's (1,300,.) outputs: the boxes divided by image_scale in float32, walked
    until the first score below score_threshold, truncated to int.  Returns (list of (box int[4], score, label), the score that
    ended the walk or None)."""
    boxes = np.asarray(boxes, np.float32) / np.float32(image_scale)
    kept = []
    for box, score, label in zip(boxes[0], np.asarray(scores)[0], np.asarray(labels)[0]):
        if score < score_threshold:
            return kept, score
        kept.append((box.astype(int), float(score), int(label)))
    return kept, None


def _caption_text(labels_to_names, score, label):
    return "{} {:.3f}".format(labels_to_names[int(label)], score)


def _render_names(result_dir, image_name):
    """render_detections' directories (created) and file names: (crop(k), no_detection(score), page)."""
    import os
    head, tail = os.path.splitext(image_name)
    cropped, in_image = os.path.join(result_dir, "detections_cropped"), os.path.join(result_dir, "detections_inImage")
    os.makedirs(cropped, exist_ok=True)
    os.makedirs(in_image, exist_ok=True)
    return (lambda k: os.path.join(cropped, "{}_{}{}".format(head, k, tail)),
            lambda score: os.path.join(cropped, "{}_{}_{}{}".format(head, "noDete_minScore-", score, tail)),
            os.path.join(in_image, image_name))


def render_detections(processed_page, draw, boxes, scores, labels, image_scale, result_dir, image_name, labels_to_names=None,
                      score_threshold=0.6):
    """The output step of test_image (RetinaNet.py:366-402) for one page.  boxes/scores/labels: the (1,300,·) detections of the
    page at network scale (score-descending).  Divides the boxes by image_scale, walks them until the first score below
    score_threshold, draws box + caption on `draw` (the original page, modified in place), and writes
    result_dir/detections_cropped/<head>_<k><tail> per table (cropped AFTER the box outline is drawn, as the reference does),
    <head>_noDete_minScore-_<score><tail> when the first detection already fails, and result_dir/detections_inImage/<image_name>.
    Returns the list of kept (box int[4], score, label)."""
    labels_to_names = labels_to_names or {0: 'table'}
    crop_name, none_name, page_name = _render_names(result_dir, image_name)
    kept, ended = _kept_detections(boxes, scores, labels, image_scale, score_threshold)
    if not kept and ended is not None:
        write_image(none_name(ended), draw)
    for k, (b, score, label) in enumerate(kept):
        draw_box(draw, b, color=label_color(label))
        write_image(crop_name(k), extract_box(draw, b))
        draw_caption(draw, b, _caption_text(labels_to_names, score, label))
    write_image(page_name, draw)
    return kept


# ---- the same step on the device: csrc/rtn_render.hip paints every crop and annotated page of a batch in one launch,
# write_images_bgr's encoders turn them into files ------------------------------------------------------------------------------------
_RENDER_COORD = 1 << 30          # rtn_render_pages' coordinate range: far outside any page, so clamping to it changes no pixel


def _render_plan(shapes, kept, labels_to_names=None, thickness=5, font_size=5):
    """The tables of one rtn_render_pages / rtn_render_host call.  shapes: (H, W) per page; kept: per page the list
    _kept_detections returns.  A page without kept detections gets no output image.  A page with J of them gets, in this order,
    crop k (the page rectangle [max(x1,0), min(x2,W)) x [max(y1,0), min(y2,H)) with outlines 0..k and captions 0..k-1) for every k
    whose rectangle is not empty, then the whole page with all J outlines and captions.  Returns a dict: the int32 / int64 arrays
    in the C-ABI's order, `masks` (uint8: the captions' masks, one bit per pixel, rows padded to whole bytes, equal captions
    shared), `images` (per output: (page, k or None for the page, h, w, byte offset)) and `out_bytes`."""
    labels_to_names = labels_to_names or {0: 'table'}
    op_begin, boxes, captions, mask_bits, mask_pitch = [0], [], [], [], []
    out_page, out_rects, out_outlines, out_captions, out_offsets, images = [], [], [], [], [], []
    blob, seen, pos = [], {}, 0

    def clamp(v):
        return int(min(max(int(v), -_RENDER_COORD), _RENDER_COORD))

    def image(p, k, x0, y0, w, h, outlines, caps):
        nonlocal pos
        out_page.append(p)
        out_rects.append((x0, y0, w, h))
        out_outlines.append(outlines)
        out_captions.append(caps)
        out_offsets.append(pos)
        images.append((p, k, h, w, pos))
        pos += (h * w * 3 + 255) & ~255

    for p, ((H, W), dets) in enumerate(zip(shapes, kept)):
        for k, (b, score, label) in enumerate(dets):
            text = _caption_text(labels_to_names, score, label)
            if text not in seen:
                mask = _caption_mask(text, font_size)
                packed = np.packbits(mask, axis=1, bitorder="little")
                seen[text] = (8 * sum(len(x) for x in blob), 8 * packed.shape[1], mask.shape[1], mask.shape[0])
                blob.append(packed.tobytes())
            bit, pitch, mw, mh = seen[text]
            x1, y1, x2, y2 = (clamp(v) for v in b)
            boxes.append((x1, y1, x2, y2))
            captions.append((x1, clamp(int(b[1]) - 10 - mh), mw, mh))
            mask_bits.append(bit)
            mask_pitch.append(pitch)
            cx0, cy0, cx1, cy1 = max(x1, 0), max(y1, 0), min(x2, W), min(y2, H)
            if cx0 < cx1 and cy0 < cy1:
                image(p, k, cx0, cy0, cx1 - cx0, cy1 - cy0, k + 1, k)
        if dets:
            image(p, None, 0, 0, W, H, len(dets), len(dets))
        op_begin.append(len(boxes))
    i32 = lambda v, shape: np.ascontiguousarray(v, np.int32).reshape(shape)
    return {
        "heights": i32([s[0] for s in shapes], (-1,)), "widths": i32([s[1] for s in shapes], (-1,)), "op_begin": i32(op_begin, (-1,)),
        "boxes": i32(boxes, (-1, 4)), "captions": i32(captions, (-1, 4)), "mask_bits": np.ascontiguousarray(mask_bits, np.int64),
        "mask_pitch": i32(mask_pitch, (-1,)), "masks": np.frombuffer(b"".join(blob), np.uint8),
        "out_page": i32(out_page, (-1,)), "out_rects": i32(out_rects, (-1, 4)), "out_outlines": i32(out_outlines, (-1,)),
        "out_captions": i32(out_captions, (-1,)), "out_offsets": np.ascontiguousarray(out_offsets, np.int64),
        "thickness": int(thickness), "images": images, "out_bytes": pos,
    }


def _render_args(plan, page_ptrs, masks_ptr, out_ptr):
    """The arguments rtn_render_pages (behind the handle, before the workspace), rtn_render_host and rtn_render_tiles_host share."""
    import ctypes as C
    n = len(page_ptrs)
    ptr = lambda a: a.ctypes.data if a.size else None
    return [n, (C.c_void_p * max(n, 1))(*page_ptrs), ptr(plan["heights"]), ptr(plan["widths"]), plan["op_begin"].ctypes.data,
            len(plan["boxes"]), ptr(plan["boxes"]), ptr(plan["captions"]), ptr(plan["mask_bits"]), ptr(plan["mask_pitch"]),
            masks_ptr, plan["masks"].size, len(plan["images"]), ptr(plan["out_page"]), ptr(plan["out_rects"]),
            ptr(plan["out_outlines"]), ptr(plan["out_captions"]), ptr(plan["out_offsets"]), plan["thickness"], out_ptr,
            plan["out_bytes"]]


def _render_files(plan, kept, ended, sources, rendered, result_dir, image_names):
    """(paths, images) of the files render_detections writes for the pages of a plan, in its order: `sources` the pages as they
    came, `rendered` the output images of plan["images"].  A crop whose rectangle is empty has no file."""
    by_page = {}
    for (p, k, _h, _w, _off), img in zip(plan["images"], rendered):
        by_page.setdefault(p, {})[k] = img
    paths, images = [], []
    for p, name in enumerate(image_names):
        crop_name, none_name, page_name = _render_names(result_dir, name)
        mine = by_page.get(p, {})
        if not kept[p] and ended[p] is not None:
            paths.append(none_name(ended[p]))
            images.append(sources[p])
        for k in range(len(kept[p])):
            if k in mine:
                paths.append(crop_name(k))
                images.append(mine[k])
        paths.append(page_name)
        images.append(mine[None] if kept[p] else sources[p])
    return paths, images


def _render_device(plan, pages):
    """One rtn_render_pages launch on the current stream for the plan's images over the CUDA pages -> (the output buffer, its
    (h, w, 3) views in the order of plan["images"]); (None, []) for a plan without images."""
    if not plan["images"]:
        return None, []
    out = torch.empty(plan["out_bytes"], dtype=torch.uint8, device=pages[0].device)
    masks = torch.from_numpy(plan["masks"].copy()).to(out.device) if plan["masks"].size else None
    args = _render_args(plan, [p.data_ptr() for p in pages], masks.data_ptr() if masks is not None else None, out.data_ptr())
    _pages.Device(out.device).call("rtn_render_pages", args,
                                   lambda: L.lib.rtn_render_workspace_bytes(len(pages), len(plan["boxes"]), len(plan["images"])))
    return out, [out[off:off + hh * ww * 3].view(hh, ww, 3) for (_p, _k, hh, ww, off) in plan["images"]]


def render_detections_device(draw_pages, boxes, scores, labels, image_scales, result_dir, image_names, labels_to_names=None,
                             score_threshold=0.6, png="host", return_pages=False):
    """render_detections for a batch of pages that live on the device.  draw_pages: list of CUDA uint8 (H,W,3) B,G,R pages (what
    read_images_bgr returns; sizes may differ; never written); boxes, scores, labels: the (B,300,·) detections, CUDA or host;
    image_scales and image_names: one per page.  The detections come to the host in one copy, the kept list of every page is
    render_detections' (the same helper), one rtn_render_pages launch paints all crops and annotated pages of the batch into one
    buffer (csrc/rtn_render.hip), and one write_images_bgr(..., png=png) call writes all files of the batch under
    render_detections' names: .jpg names at cv2.imwrite's quality 95, 4:2:0 through the device encoder.  A page without a kept
    detection is written as it came.  One difference from render_detections: crop k is the page rectangle
    [max(x1,0), min(x2,W)) x [max(y1,0), min(y2,H)); where that is empty no file is written for k (render_detections raises inside
    Pillow) and the numbering of the others stays.  Returns the kept list per page; with return_pages=True also, per page, (list
    of the crops as CUDA tensors, None for an empty one; the annotated page), the source page itself where nothing was kept."""
    pages = list(draw_pages)
    image_names = list(image_names)
    for i, p in enumerate(pages):
        if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.uint8 and p.dim() == 3 and p.shape[2] == 3
                and p.shape[0] >= 1 and p.shape[1] >= 1):
            raise ValueError("page %d: a CUDA uint8 (H,W,3) tensor expected, got %s" % (
                i, "%s %s" % (p.dtype, tuple(p.shape)) if isinstance(p, torch.Tensor) else type(p).__name__))
    host3 = []
    if any(isinstance(a, torch.Tensor) and a.is_cuda for a in (boxes, scores, labels)):
        torch.cuda.synchronize()                    # Engine.detect may have run on a stream of its own (in_flight > 1)
    for a in (boxes, scores, labels):
        host3.append(a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a))
    boxes, scores, labels = host3
    if not (len(pages) == len(image_names) == len(image_scales) == len(boxes) == len(scores) == len(labels)):
        raise ValueError("%d pages, %d names, %d scales, %d / %d / %d detection rows" % (
            len(pages), len(image_names), len(image_scales), len(boxes), len(scores), len(labels)))
    kept, ended = [], []
    for i in range(len(pages)):
        k, e = _kept_detections(boxes[i:i + 1], scores[i:i + 1], labels[i:i + 1], image_scales[i], score_threshold)
        kept.append(k)
        ended.append(e)
    pages = [p.contiguous() for p in pages]
    plan = _render_plan([(p.shape[0], p.shape[1]) for p in pages], kept, labels_to_names)
    rendered = _render_device(plan, pages)[1]
    paths, images = _render_files(plan, kept, ended, pages, rendered, result_dir, image_names)
    write_images_bgr(paths, images, png=png)
    if not return_pages:
        return kept
    per_page = [([None] * len(k), p) for k, p in zip(kept, pages)]
    for (p, k, _h, _w, _off), img in zip(plan["images"], rendered):
        if k is None:
            per_page[p] = (per_page[p][0], img)
        else:
            per_page[p][0][k] = img
    return kept, per_page


def _render_batch(draw_pages, boxes, scores, labels, scales, result_dir, names, labels_to_names, score_threshold, png, headers):
    """The output step of one batch that detect_files and detect_raw_files share: render_detections_device, and with headers=True
    HeaderDetect.py's step on the crops while they are on the device.  Returns the kept list of every page."""
    import os
    got = render_detections_device(draw_pages, boxes, scores, labels, scales, result_dir, names, labels_to_names=labels_to_names,
                                   score_threshold=score_threshold, png=png, return_pages=headers)
    if not headers:
        return got
    from . import header
    got, per_page = got
    crops, crop_names = [], []
    for name, (page_crops, _page) in zip(names, per_page):
        crop_name = _render_names(result_dir, name)[0]
        for k, crop in enumerate(page_crops):
            if crop is not None:
                crops.append(crop)
                crop_names.append(crop_name(k))
    out_dir = os.path.join(result_dir, "headerResults")
    fits = [header.sampled_points(c.shape[0], c.shape[1]) <= header.MAX_POINTS for c in crops]
    for c, name, ok in zip(crops, crop_names, fits):
        if not ok:                          # a sliver of a box: 500 x dh points past the limit; its OrigImage.png alone is written
            warnings.warn("header detection skipped for %s: %d x %d is too tall for a width of 500" % (name, c.shape[0], c.shape[1]))
    found = iter(header.detect_headers([c for c, ok in zip(crops, fits) if ok]))
    paths, images = header._header_outputs(crops, crop_names, [next(found) if ok else None for ok in fits], out_dir)
    write_images_bgr(paths, images, png=png)
    return got


def _cells_batch(pages, kept, result_dir, names):
    """cells=True of detect_files and detect_raw_files for one batch: table_cells on the kept boxes, the CSVs under cellResults."""
    import os
    from . import structure
    boxes = [np.array([b for b, _score, _label in k], np.float64).reshape(-1, 4) for k in kept]
    structure.write_csvs(structure.table_cells(pages, boxes), names, os.path.join(result_dir, "cellResults"))


def detect_files(model, src_paths, orig_paths, result_dir, batch_size=8, score_threshold=0.6, labels_to_names=None, png="host",
                 min_side=800, max_side=1333, headers=False, cells=False):
    """The loop of RetinaNet.py's test() over files, in batches of batch_size, with every pixel on the device: read_images_bgr of
    the preprocessed pages (src_paths) and of the pages to draw on (orig_paths), compute_inputs_device, the inference model's
    engine().detect, render_detections_device with image_names = basename(src_paths).  `model`: a retinanet_bbox model (ValueError
    otherwise).  headers=True also runs HeaderDetect.py's step on the crops of every batch while they are on the device
    (model/header.py detect_headers) and writes its files under result_dir/headerResults/test_<crop file name without extension>/;
    a crop too tall for detect_headers' point limit is skipped with a warning.  cells=True also runs model/structure.py's
    table_cells on every batch's pages (those drawn on) and kept boxes while they are on the device and writes
    result_dir/cellResults/<name without extension>_table<k>_cells.csv for kept box k; cells=False changes no byte of the outputs.
    Returns the kept list of every file."""
    import os
    from . import preprocess
    from .page_io import read_images_bgr
    if not getattr(model, "bbox", False):
        raise ValueError("detect_files: the inference model (retinanet_bbox) is required")
    src_paths, orig_paths = list(src_paths), list(orig_paths)
    if len(src_paths) != len(orig_paths):
        raise ValueError("%d preprocessed pages for %d pages to draw on" % (len(src_paths), len(orig_paths)))
    if int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    dtype = torch.float32 if model._root().dtype == "f32" else torch.bfloat16
    eng = model.engine()
    kept = []
    for i in range(0, len(src_paths), int(batch_size)):
        src, orig = src_paths[i:i + int(batch_size)], orig_paths[i:i + int(batch_size)]
        canvas, scales = preprocess.compute_inputs_device(read_images_bgr(src), min_side=min_side, max_side=max_side, dtype=dtype)
        boxes, scores, labels = eng.detect(canvas, nms=model.nms, class_specific_filter=model.class_specific_filter)
        names = [os.path.basename(p) for p in src]
        pages = read_images_bgr(orig)
        kept += _render_batch(pages, boxes, scores, labels, scales, result_dir, names, labels_to_names, score_threshold, png, headers)
        if cells:
            _cells_batch(pages, kept[i:], result_dir, names)
    return kept


def _raw_batch(model, eng, dtype, pages, factors, names, result_dir, score_threshold, labels_to_names, png, min_side, max_side, headers,
               deskew, cells):
    """The body of one batch that detect_raw_files and detect_pdf_files share, from the pages as they were read (CUDA tensors) to the
    files: deskew, interpolate_images where a factor is not 1, the distance maps, the network's inputs, detect, the output step and
    the cells.  Returns (the kept list of every page, the deskew angles or None, the (H, W) of every page as it was read)."""
    from . import preprocess
    pages = list(pages)
    sizes = [(int(p.shape[0]), int(p.shape[1])) for p in pages]
    angles = None
    if deskew:
        pages, angles = preprocess.deskew_images(pages)
    grow = [k for k, f in enumerate(factors) if f != 1.0]
    if grow:
        for k, big in zip(grow, preprocess.interpolate_images([pages[k] for k in grow], [factors[k] for k in grow])):
            pages[k] = big
    processed = preprocess.preprocess_device_pages(pages)
    canvas, scales = preprocess.compute_inputs_device(processed, min_side=min_side, max_side=max_side, dtype=dtype)
    boxes, scores, labels = eng.detect(canvas, nms=model.nms, class_specific_filter=model.class_specific_filter)
    kept = _render_batch(pages, boxes, scores, labels, scales, result_dir, names, labels_to_names, score_threshold, png, headers)
    if cells:
        _cells_batch(pages, kept, result_dir, names)
    return kept, angles, sizes


def detect_raw_files(model, orig_paths, result_dir, factors=None, batch_size=8, score_threshold=0.6, labels_to_names=None, png="host",
                     min_side=800, max_side=1333, headers=False, deskew=False, cells=False):
    """Raw scans to detections in one call, in batches of batch_size, with every pixel on the device: read_images_bgr of the scans,
    interpolate_images where a page's factor is not 1 (factors: one per file, by default preprocess.interpolation_factor of its
    base name: 4.17 for "-72.jpg", 3 for "-100.jpg"), preprocess_device_pages (the distance maps), compute_inputs_device, the
    inference model's engine().detect, and detect_files' output step on the (enlarged) pages with image_names =
    basename(orig_paths); headers=True as in detect_files.  `model`: a retinanet_bbox model (ValueError otherwise).
    deskew=True rotates every page upright right after it is read (preprocess.deskew_images with its defaults); everything after,
    the rendered pages included, is the deskewed page, and the boxes are in its coordinates (preprocess.boxes_to_scan maps them back).
    cells=True as in detect_files, on the (deskewed, enlarged) pages the boxes belong to: with deskew=True the grid is taken on the
    upright page and the CSV coordinates are those of the upright page.
    Unlike the reference's flow (interpolateImages, preProcessSampleImages, then test() on the written files), the enlarged and the
    processed page never pass through a JPEG file: the results are those of that flow with lossless (PNG) intermediate files.
    Returns the kept list of every file."""
    import os
    from . import preprocess
    from .page_io import read_images_bgr
    if not getattr(model, "bbox", False):
        raise ValueError("detect_raw_files: the inference model (retinanet_bbox) is required")
    orig_paths = list(orig_paths)
    if factors is None:
        factors = [preprocess.interpolation_factor(os.path.basename(str(p))) for p in orig_paths]
    factors = [float(f) for f in factors]
    if len(factors) != len(orig_paths):
        raise ValueError("%d factors for %d pages" % (len(factors), len(orig_paths)))
    if int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    dtype = torch.float32 if model._root().dtype == "f32" else torch.bfloat16
    eng = model.engine()
    kept = []
    for i in range(0, len(orig_paths), int(batch_size)):
        orig, fs = orig_paths[i:i + int(batch_size)], factors[i:i + int(batch_size)]
        names = [os.path.basename(str(p)) for p in orig]
        kept += _raw_batch(model, eng, dtype, read_images_bgr(orig), fs, names, result_dir, score_threshold, labels_to_names, png,
                           min_side, max_side, headers, deskew, cells)[0]
    return kept


def detect_pdf_files(model, pdf_paths, result_dir, pages=None, factors=None, batch_size=8, score_threshold=0.6, labels_to_names=None, png="host",
                     min_side=800, max_side=1333, headers=False, deskew=False, cells=False):
    """Scanned PDFs to detections in one call: detect_raw_files' loop with its pages coming from model/pdf.py's read_pdfs_pages (DESIGN
    §3.4p) instead of read_images_bgr.  The pages of all files are read in one device batch and then go through the network in batches
    of batch_size, whatever file they belong to.  pages: None, or per file the page indices (from 0) to read (None: all); factors:
    None (1.0 for every page) or one enlargement factor per read page, in file and page order.  The image name of page k (from 1) of
    <stem>.pdf is the reference's convertPdfsToImages name, "<stem>_Page<k>-<dpi>.png" with dpi = round(72 sx); the rendered files are
    detect_raw_files' under those names.  A page that is not image-only (or that no decoder takes) is skipped with a warning.  Besides
    the rendered files, result_dir/pdfResults/<stem>_tables.csv holds every kept box of a file in the reference's PDF-CSV layout
    (header image_id,xmin,ymin,xmax,ymax,label; image_id "<stem>_Page<k>") in integer points of the unrotated page, y upwards
    (pdf.boxes_to_pdf, truncated as PDFCSVtoImageCSV truncates); with deskew=True the boxes are first mapped back to the scan by
    preprocess.boxes_to_scan.  Returns a list of (path, page_index, kept), kept None for a skipped page, in file and page order."""
    import csv
    import os
    from . import pdf, preprocess
    if not getattr(model, "bbox", False):
        raise ValueError("detect_pdf_files: the inference model (retinanet_bbox) is required")
    pdf_paths = list(pdf_paths)
    if int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    labels_to_names = labels_to_names or {0: 'table'}
    read, infos = pdf.read_pdfs_pages(pdf_paths, pages=pages, return_info=True)
    out, todo = [], []                                             # todo: (position in out, file, PdfPage, tensor)
    for f, (path, tensors, info) in enumerate(zip(pdf_paths, read, infos)):
        want = None if pages is None or pages[f] is None else set(int(v) for v in pages[f])
        for page, t in zip(info.pages, tensors):
            if want is not None and page.index not in want:
                continue
            if t is None:
                warnings.warn("%s, page %d skipped: %s" % (path, page.index + 1, page.refused))
            else:
                todo.append((len(out), f, page, t))
            out.append((path, page.index, None))
    factors = [1.0] * len(todo) if factors is None else [float(v) for v in factors]
    if len(factors) != len(todo):
        raise ValueError("%d factors for %d pages" % (len(factors), len(todo)))
    dtype = torch.float32 if model._root().dtype == "f32" else torch.bfloat16
    eng = model.engine()
    rows = {f: [] for f in range(len(pdf_paths))}
    stem = lambda f: os.path.splitext(os.path.basename(str(pdf_paths[f])))[0]
    for i in range(0, len(todo), int(batch_size)):
        batch, fs = todo[i:i + int(batch_size)], factors[i:i + int(batch_size)]
        names = ["%s_Page%d-%d.png" % (stem(f), page.index + 1, int(round(72 * page.sx))) for _pos, f, page, _t in batch]
        kept, angles, sizes = _raw_batch(model, eng, dtype, [t for _pos, _f, _page, t in batch], fs, names, result_dir, score_threshold,
                                         labels_to_names, png, min_side, max_side, headers, deskew, cells)
        for k, ((pos, f, page, _t), mine, factor) in enumerate(zip(batch, kept, fs)):
            out[pos] = (out[pos][0], page.index, mine)
            boxes = np.array([b for b, _score, _label in mine], np.float64).reshape(-1, 4)
            if deskew and len(boxes):
                boxes = preprocess.boxes_to_scan(boxes / factor, angles[k], sizes[k][0], sizes[k][1]) * factor
            for (x1, y1, x2, y2), (_b, _score, label) in zip(pdf.boxes_to_pdf(boxes, page, factor=factor), mine):
                rows[f].append(("%s_Page%d" % (stem(f), page.index + 1), int(x1), int(y1), int(x2), int(y2), labels_to_names[int(label)]))
    os.makedirs(os.path.join(result_dir, "pdfResults"), exist_ok=True)
    for f in range(len(pdf_paths)):
        with open(os.path.join(result_dir, "pdfResults", stem(f) + "_tables.csv"), "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["image_id", "xmin", "ymin", "xmax", "ymax", "label"])
            w.writerows(rows[f])
    return out
