"""connectedComponentAnalysis.py of the reference on the device: is a scan too coarse, and how tall is its text?
process_graphical_lines finds the ruling lines of a page and paints them out; process_image measures the heights of the text
lines that remain; main() bins the heights into 25 bins over 0 .. 100.  Launches per batch of pages (csrc/rtn_cca.hip): the two
line masks (threshold, transpose, row openings, transpose back), labelling (tiles in LDS, merge, flatten, frame and external
flags, count, scan, rank, boxes, finish), paint; then the text mask (one launch), labelling again and, when asked for, the
outlines.  Counts and boxes come to the host between the stages; the histogram is host arithmetic.

OpenCV is not a dependency and was not at hand when this was written: the rules below restate its published behaviour (BGR2GRAY,
adaptiveThreshold's rounded mean, the morphology border that ignores positions outside the image, GaussianBlur's 8-bit fixed
point, findContours(RETR_EXTERNAL) + boundingRect) from memory, recalled and not verifiable offline.  They are the specification:
  * gray = (1868 b + 9617 g + 4899 r + 8192) >> 14; a gray page is taken as it is.
  * process_graphical_lines: g = 255 - gray; S = the 15x15 box sum of g with replicated borders; bw = 255 where
    g - (2 S + 225) // 450 > 2; horizontal = bw eroded, then dilated, along x by the window [x - L // 2, x - L // 2 + L - 1] cut to
    the image, L = W // 30; vertical the same along y with L = H // 30; the box of every external component of horizontal, then of
    vertical, becomes 255 in every channel.
  * process_image: blur with the taps (27, 202, 27) / 256 (exp(-x^2 / 0.5) normalised, times 256, rounded, the centre taking the
    remainder; the outer two of the five taps are 0), BORDER_REFLECT_101, 16 bits kept after the row pass, (sum + 32768) >> 16
    after the column pass; black-hat with the 1x4 element (window [x - 2, x + 1]); > 10; dilate; close twice with the 1x10 element
    (window [x - 5, x + 4]).  The reference asks for 9 iterations of a 1x4 "cross", which is all ones: OpenCV folds the iterations
    into one 1x28 element anchored at 18 (window [x - 18, x + 9]), and with ignored borders that equals the iterated form.
  * external components: foreground 8-connected, background 4-connected with the page inside a one-pixel background frame; a
    component is external iff one of its pixels is 4-adjacent to the background region that contains the frame; its box is the
    bounding box of its pixels; components are ordered by the raster index y * W + x of their first pixel.

Differences from the reference:
  * the intermediate Temp/*_0 .. 8 images are not written (analyse_files writes <name>_3.Final.jpg and <name>_9.Final.jpg);
  * the matplotlib histogram figure is not drawn (height_histogram gives its counts and the mode bin main() prints);
  * main()'s random choice of three images and its LR / HR file-name pairing are the caller's: analyse_files takes paths;
  * interpolateImages is not provided;
  * findContours' own order of the contours is replaced by the raster order of the first pixels, which no scheduling changes;
  * pages with a side below 30 (the reference fails: its structuring element has length 0) or above 16384 raise ValueError."""
import os

import numpy as np

from . import _pages, _rt
from ._pages import Device as _Device, Twins as _Twins, i32 as _i32, pointers as _pointers, ptr as _ptr, starts as _starts

L = _rt.L

MIN_SIDE = 30
MAX_SIDE = 16384
BINS, RANGE = 25, (0, 100)               # drawPDFHist: num_bins, _range
FILL, OUTLINE = 0, 1                     # rtn_cca_paint modes


def max_components(h, w):
    """The most 8-connected components an h x w image can hold: one pixel on every second row and column."""
    return ((int(h) + 1) // 2) * ((int(w) + 1) // 2)


def _backend(pages, device):
    if not device:
        return _Twins()
    return _Device(pages[0].device) if pages else None


def _check_batch(pages, device):
    """The pages of a public call, CUDA tensors on the device path and NumPy arrays for the twins -> (pages, [(h, w, channels)])."""
    return _pages.check_pages(pages, MIN_SIDE, MAX_SIDE, device, upload=False)


def _workspace(hs, ws, n_boxes=0):
    return lambda: L.lib.rtn_cca_workspace_bytes(len(hs), _ptr(hs), _ptr(ws), n_boxes)


def _layout(shapes):
    hs, ws, ch = _i32([s[0] for s in shapes]), _i32([s[1] for s in shapes]), _i32([s[2] for s in shapes])
    return (hs, ws, ch) + _starts(hs.astype(np.int64) * ws)


def _lines_mask(be, pages, shapes, bw=False):
    """-> the packed horizontal and vertical masks (and, from the twins with bw=True, the thresholded image) and the offsets."""
    hs, ws, ch, off, total = _layout(shapes)
    hor, ver = be.empty(total), be.empty(total)
    extra = ()
    if not be.device:
        extra = (be.empty(total),) if bw else (None,)
    be.call("rtn_cca_lines_mask", [len(pages), _pointers(be, pages), _ptr(hs), _ptr(ws), _ptr(ch), _ptr(off), be.ptr(hor), be.ptr(ver),
                                   total], _workspace(hs, ws), extra=tuple(None if e is None else be.ptr(e) for e in extra))
    return (hor, ver, off) + ((extra[0],) if bw else ())


def _text_mask(be, pages, shapes, stages=False):
    """-> the packed closed mask (and, from the twins with stages=True, the four earlier planes of every page) and the offsets."""
    hs, ws, ch, off, total = _layout(shapes)
    closed = be.empty(total)
    extra = ()
    if not be.device:
        extra = (be.empty(4 * total),) if stages else (None,)
    be.call("rtn_cca_text_mask", [len(pages), _pointers(be, pages), _ptr(hs), _ptr(ws), _ptr(ch), _ptr(off), be.ptr(closed), total],
            _workspace(hs, ws), extra=tuple(None if e is None else be.ptr(e) for e in extra))
    return (closed, off) + ((extra[0],) if stages else ())


def _label(be, images, sizes, external_only=True, capacity=None):
    """The components of binary images [(h, w) uint8] -> one int32 (n, 4) array of x, y, w, h per image, in the order of the first
    pixels.  capacity: boxes per image; None gives every image room for max_components, which cannot overflow.  RtnError
    (RTN_EINVAL) when an image holds more components than its capacity."""
    n = len(images)
    hs, ws = _i32([s[0] for s in sizes]), _i32([s[1] for s in sizes])
    cap = _i32([max_components(h, w) for h, w in zip(hs, ws)] if capacity is None else capacity)
    first, room = _starts(cap)
    counts, boxes = be.empty(max(n, 1), np.int32), be.empty(4 * max(room, 1), np.int32)
    be.call("rtn_cca_label", [n, _pointers(be, images), _ptr(hs), _ptr(ws), int(bool(external_only)), _ptr(cap), _ptr(first),
                              be.ptr(counts), be.ptr(boxes), 16 * max(room, 1)], _workspace(hs, ws))
    counts_h = be.host(counts)[:n]
    out = []
    for i in range(n):
        b = boxes[4 * int(first[i]):4 * (int(first[i]) + int(counts_h[i]))]
        out.append(np.array(be.host(b), np.int32).reshape(-1, 4))
    return out


def _paint(be, pages, shapes, boxes, mode):
    """Paints boxes[i] ((n, 4) x, y, w, h) into pages[i] in place: FILL or OUTLINE."""
    hs, ws, ch, _off, _total = _layout(shapes)
    page = _i32(np.concatenate([np.full(len(b), i) for i, b in enumerate(boxes)]) if boxes else [])
    flat = _i32(np.concatenate([np.reshape(b, (-1, 4)) for b in boxes]) if boxes else np.zeros((0, 4)))
    if not len(page):
        return
    be.call("rtn_cca_paint", [len(pages), _pointers(be, pages), _ptr(hs), _ptr(ws), _ptr(ch), len(page), _ptr(page), _ptr(flat), mode],
            _workspace(hs, ws, len(page)))


def _mask_views(be, buf, off, shapes):
    return [be.view(buf, int(o), (s[0], s[1])) for o, s in zip(off, shapes)]


def _remove(be, pages, shapes):
    if not pages:
        return [], []
    hor, ver, off = _lines_mask(be, pages, shapes)
    images = _mask_views(be, hor, off, shapes) + _mask_views(be, ver, off, shapes)
    found = _label(be, images, [s[:2] for s in shapes] * 2)
    n = len(pages)
    boxes = [np.concatenate([found[i], found[n + i]]) for i in range(n)]
    cleaned = [be.clone(p) for p in pages]
    _paint(be, cleaned, shapes, boxes, FILL)
    return cleaned, boxes


def _text(be, pages, shapes):
    if not pages:
        return []
    closed, off = _text_mask(be, pages, shapes)
    return _label(be, _mask_views(be, closed, off, shapes), [s[:2] for s in shapes])


def kept_boxes(boxes):
    """process_image's filter: the boxes with w > h and h > 0 and w * h > 500, in box order."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    return np.asarray(boxes, np.int32).reshape(-1, 4)[(b[:, 2] > b[:, 3]) & (b[:, 3] > 0) & (b[:, 2] * b[:, 3] > 500)]


def _heights(be, pages, shapes, annotate):
    kept = [kept_boxes(b) for b in _text(be, pages, shapes)]
    heights = [k[:, 3].copy() for k in kept]
    if not annotate:
        return heights
    drawn = [be.clone(p) for p in pages]
    if pages:
        _paint(be, drawn, shapes, kept, OUTLINE)
    return heights, drawn


def remove_graphical_lines(pages, device=True):
    """process_graphical_lines for a batch.  pages: uint8 (H,W,3) B,G,R or (H,W) gray, of any mix of sizes with sides 30 .. 16384;
    CUDA tensors (never written), or NumPy arrays with device=False (the CPU twins, no GPU needed).  Returns (cleaned_pages,
    line_boxes): new pages with the box of every ruling line painted white, and per page the int32 (n, 4) boxes x, y, w, h, the
    horizontal lines' first.  ValueError naming the page, before anything is launched, for a side outside 30 .. 16384."""
    pages, shapes = _check_batch(pages, device)
    return _remove(_backend(pages, device), pages, shapes)


def text_components(pages, device=True):
    """process_image up to boundingRect: per page the int32 (n, 4) boxes x, y, w, h of all external components of the closed
    image, in the order of their first pixels."""
    pages, shapes = _check_batch(pages, device)
    return _text(_backend(pages, device), pages, shapes)


def component_heights(pages, annotate=False, device=True):
    """process_image: per page the int32 heights of the text components with w > h and h > 0 and w * h > 500, in box order.
    annotate=True returns (heights, annotated_pages): new pages with those boxes outlined from (x, y) to (x + w, y + h) in
    (0, 255, 0) (255 on a gray page), thickness 2, by the band rule of draw_box."""
    pages, shapes = _check_batch(pages, device)
    return _heights(_backend(pages, device), pages, shapes, annotate)


def height_histogram(heights):
    """drawPDFHist for one list of heights: (counts[25], mode_lo, mode_hi) with np.histogram(heights, 25, (0, 100))'s semantics
    (bins of 4, the last one closed at 100, values outside ignored); the mode is the first bin that holds the largest count."""
    counts = np.zeros(BINS, np.int64)
    size = (RANGE[1] - RANGE[0]) // BINS
    for v in np.asarray(heights).reshape(-1):
        if RANGE[0] <= v <= RANGE[1]:
            counts[min(int((v - RANGE[0]) * BINS / (RANGE[1] - RANGE[0])), BINS - 1)] += 1
    lo = RANGE[0] + int(np.argmax(counts)) * size
    return counts, lo, lo + size


def _analyse(be, pages, shapes, annotate):
    cleaned, line_boxes = _remove(be, pages, shapes)
    got = _heights(be, cleaned, shapes, annotate)
    heights, drawn = got if annotate else (got, [None] * len(pages))
    out = []
    for i in range(len(pages)):
        counts, lo, hi = height_histogram(heights[i])
        out.append({"line_boxes": line_boxes[i], "cleaned": cleaned[i], "heights": heights[i], "histogram": counts,
                    "mode_bin": (lo, hi)})
        if annotate:
            out[-1]["annotated"] = drawn[i]
    return out


def analyse_scan(pages, annotate=False, device=True):
    """main()'s chain for every page: remove_graphical_lines, component_heights on the cleaned page, height_histogram.  One dict
    per page: line_boxes, cleaned (the page without its ruling lines), heights, histogram (25 counts), mode_bin (lo, hi), and with
    annotate=True annotated (the cleaned page with the kept boxes outlined)."""
    pages, shapes = _check_batch(pages, device)
    return _analyse(_backend(pages, device), pages, shapes, annotate)


def analyse_files(paths, result_dir=None, png="host"):
    """analyse_scan over image files read by read_images_bgr.  With result_dir, writes <name>_3.Final.jpg (the cleaned page) and
    <name>_9.Final.jpg (the annotated page) there, <name> the file's base name as main() passes it, through
    write_images_bgr(..., png=png).  Returns analyse_scan's dicts (with annotated when result_dir is given)."""
    from .page_io import read_images_bgr, write_images_bgr
    paths = list(paths)
    results = analyse_scan(read_images_bgr(paths), annotate=result_dir is not None)
    if result_dir is not None:
        os.makedirs(result_dir, exist_ok=True)
        out_paths, images = [], []
        for path, res in zip(paths, results):
            name = os.path.basename(str(path))
            out_paths += [os.path.join(result_dir, "{}_3.Final.jpg".format(name)), os.path.join(result_dir, "{}_9.Final.jpg".format(name))]
            images += [res["cleaned"], res["annotated"]]
        write_images_bgr(out_paths, images, png=png)
    return results
