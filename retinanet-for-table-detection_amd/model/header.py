"""HeaderDetect.py of the reference on the device: for each table crop, resize to a width of 500, convert to HSV,
fit k-means for k = 1 .. 9, pick k at the elbow, describe every cluster by its channel statistics and cut one patch per cluster
out of the crop by the cluster's Q1 .. Q3 range.  Four launches per batch of crops (csrc/rtn_header.hip): sample, cluster (one
workgroup per crop runs the nine fits in a chain), stats (histograms of the chosen k) and patches; the nine distortions and the
histograms come to the host, where opt_k and the statistics are a few hundred float64 operations.

Differences from the reference:
  * k-means starts from a deterministic variance split instead of sklearn's k-means++ with random_state=0: the fit for k + 1 starts
    from the fit for k, with the cluster of the largest SSE split along its channel of the largest variance, and a fit has converged
    when no label changes (sklearn also stops on a centre shift below tol).  Distances and centres are float32, all sums integers.
  * imutils.resize(width=500) is an exact box filter in both directions (cv2 uses INTER_AREA, which interpolates when enlarging).
  * kneed is not used: k is optK's pick (the reference computes both and uses kneed's), 5 (extractDominantColor's default) when
    optK gives None.
  * Optimal_K.png and the matplotlib PDF histograms are not written.
  * The dominant-colour list is ordered by count with ties to the lower index (Counter.most_common orders sklearn's clusters).
  * Std is taken from the histogram as sqrt(sum(hist * (v - mean)^2) / n) in float64: NumPy's own sum over the raw list rounds in
    another order, which can show after .astype(int) only where the exact value is an integer.
The colour conversions restate OpenCV's 8-bit BGR2HSV / HSV2BGR from its published source (recalled, not verifiable offline)."""
import colorsys
import os

import numpy as np
import torch

from . import _pages, _rt
from ._pages import Device as _Device, Twins as _Twins, pointers as _pointers, ptr as _ptr, starts as _starts

L = _rt.L

WIDTH = L.RTN_HEADER_WIDTH
MAX_K = L.RTN_HEADER_MAX_K
MAX_POINTS = L.RTN_HEADER_MAX_POINTS
DEFAULT_K = 5                      # extractDominantColor(number_of_colors=5)
H_DIFF = 20                        # main(): a cluster is "Selected" when Q3[0] - Q1[0] < H_diff


def opt_k(distortions):
    """optK of the reference: the k (1-based) of the largest second-difference "strength" of the distortions, rounded to three
    places; None when no strength is positive."""
    d = [x / 100. for x in distortions]
    delta1 = [d[i] - d[i + 1] for i in range(len(d) - 1)]
    delta2 = [delta1[i] - delta1[i + 1] for i in range(len(delta1) - 1)]
    delta1.insert(0, None)
    delta2.insert(0, None)
    delta2.insert(0, None)
    strength = [delta2[i + 1] - delta1[i + 1] for i in range(len(d) - 1) if i > 0]
    strength.append(0)
    strength.insert(0, 0)
    strength = [round(x, 3) for x in strength]
    best = max(strength)
    return strength.index(best) + 1 if best > 0 else None


def sampled_points(h, w):
    """The points a crop of h x w is sampled to: 500 * int(h * (500 / float(w)))."""
    return WIDTH * int(int(h) * (WIDTH / float(int(w))))


def _plan(shapes):
    """The batch layout for crops of `shapes` [(h, w)]: which crops are sampled (dh = int(h * (500 / float(w))) >= 1; the others
    give None), their destination heights and their first points in the packed buffers.  ValueError for a crop past MAX_POINTS."""
    idx, hs, ws, dhs = [], [], [], []
    for i, (h, w) in enumerate(shapes):
        h, w = int(h), int(w)
        if h < 1 or w < 1 or h > 65500 or w > 65500:
            raise ValueError("crop %d: sides within 1 .. 65500 expected, got %d x %d" % (i, h, w))
        dh = int(h * (WIDTH / float(w)))
        if dh < 1:
            continue
        if WIDTH * dh > MAX_POINTS:
            raise ValueError("crop %d (%d x %d): %d x %d sampled points are more than %d" % (i, h, w, dh, WIDTH, MAX_POINTS))
        idx.append(i)
        hs.append(h)
        ws.append(w)
        dhs.append(dh)
    dst = np.asarray(dhs, np.int32)
    n = dst.astype(np.int64) * WIDTH
    offsets, total = _starts(n)
    return {"n": len(idx), "idx": idx, "heights": np.asarray(hs, np.int32), "widths": np.asarray(ws, np.int32), "dst": dst,
            "points": n, "offsets": offsets, "total": total}


def _workspace(n, n_patches=0):
    return lambda: L.lib.rtn_header_workspace_bytes(n, n_patches)


def _sample(be, plan, crops):
    """Stage 1 -> the packed H,S,V buffer (3 bytes per point)."""
    n = plan["n"]
    hsv = be.empty(3 * plan["total"])
    ptrs = _pointers(be, [crops[i] for i in plan["idx"]])
    be.call("rtn_header_sample", [n, ptrs, _ptr(plan["heights"]), _ptr(plan["widths"]), _ptr(plan["dst"]), _ptr(plan["offsets"]),
                                  be.ptr(hsv), 3 * plan["total"]], _workspace(n))
    return hsv


def _cluster(be, plan, hsv, max_iter):
    """Stage 2 -> (centres (n,9,9,3) f32, counts (n,9,9) u32, passes (n,9) i32, distortion_fx (n,9) u64, labels: 9 bytes per point)."""
    n = plan["n"]
    centres, counts = be.empty(n * MAX_K * MAX_K * 3, np.float32), be.empty(n * MAX_K * MAX_K, np.uint32)
    passes, dist = be.empty(n * MAX_K, np.int32), be.empty(n * MAX_K, np.uint64)
    labels = be.empty(MAX_K * plan["total"])
    be.call("rtn_header_cluster", [n, _ptr(plan["dst"]), _ptr(plan["offsets"]), be.ptr(hsv), 3 * plan["total"], int(max_iter),
                                   be.ptr(centres), be.ptr(counts), be.ptr(passes), be.ptr(dist), be.ptr(labels),
                                   MAX_K * plan["total"]], _workspace(n))
    return centres, counts, passes, dist, labels


def _stats(be, plan, ks, hsv, labels):
    """Stage 4 -> hist (n,9,3,256) u32 of the ks[i]-cluster fit of every crop."""
    n = plan["n"]
    ks = np.ascontiguousarray(ks, np.int32)
    hist = be.empty(n * MAX_K * 3 * 256, np.uint32)
    be.call("rtn_header_stats", [n, _ptr(plan["dst"]), _ptr(plan["offsets"]), _ptr(ks), be.ptr(hsv), 3 * plan["total"],
                                 be.ptr(labels), MAX_K * plan["total"], be.ptr(hist)], _workspace(n))
    return hist


def _patches(be, plan, hsv, patch_crop, low, high):
    """Stage 5 -> (the buffer, the byte offset of every patch) for patches [(crop, low[3], high[3])] in one launch."""
    patch_crop = np.ascontiguousarray(patch_crop, np.int32)
    low, high = np.ascontiguousarray(low, np.uint8), np.ascontiguousarray(high, np.uint8)
    sizes = plan["points"][patch_crop] * 3 if len(patch_crop) else np.zeros(0, np.int64)
    first, total = _starts(sizes)
    offs = np.append(first, total)
    out = be.empty(max(total, 1))
    be.call("rtn_header_patches", [plan["n"], _ptr(plan["dst"]), _ptr(plan["offsets"]), be.ptr(hsv), 3 * plan["total"],
                                   len(patch_crop), _ptr(patch_crop), _ptr(low), _ptr(high), _ptr(first), be.ptr(out),
                                   total], _workspace(plan["n"], len(patch_crop)))
    return out, offs


def histogram_stats(hist):
    """analyse() for one cluster from its (3, 256) histograms, in float64, as NumPy gives from the raw pixel list: min_value,
    max_value, Mean and Std (.astype(int)), Q1, Q3 and Median (np.quantile's linear rule)."""
    hist = np.asarray(hist, np.int64)
    v = np.arange(256, dtype=np.float64)
    out = {k: [] for k in ("min_value", "max_value", "Mean", "Std", "Q1", "Q3", "Median")}
    for c in range(3):
        h = hist[c]
        n = int(h.sum())
        nz = np.nonzero(h)[0]
        cum = np.cumsum(h)
        at = lambda i: int(np.searchsorted(cum, i, side="right"))            # the i-th value of the sorted list

        def quantile(q):
            virtual = (n - 1) * q
            lo = int(np.floor(virtual))
            hi = min(lo + 1, n - 1)
            t = virtual - lo
            a, b = np.float64(at(lo)), np.float64(at(hi))
            d = b - a
            return b - d * (1 - t) if t >= 0.5 else a + d * t                # numpy's _lerp

        mean = np.float64(int((h * np.arange(256)).sum())) / n
        dev = v - mean
        std = np.sqrt((h * (dev * dev)).sum() / n)
        out["min_value"].append(int(nz[0]))
        out["max_value"].append(int(nz[-1]))
        out["Mean"].append(int(mean))
        out["Std"].append(int(std))
        out["Q1"].append(quantile(0.25))
        out["Q3"].append(quantile(0.75))
        out["Median"].append((at((n - 1) // 2) + at(n // 2)) / 2.0)
    return {"min_value": np.asarray(out["min_value"], np.uint8), "max_value": np.asarray(out["max_value"], np.uint8),
            "Mean": np.asarray(out["Mean"], np.int64), "Std": np.asarray(out["Std"], np.int64),
            "Q1": np.asarray(out["Q1"], np.float64), "Q3": np.asarray(out["Q3"], np.float64),
            "Median": np.asarray(out["Median"], np.float64)}


def dominant_colours(centres, counts):
    """getColorInformation: the non-empty clusters by falling count (ties: the lower index first)."""
    total = int(np.sum(counts))
    order = sorted((j for j in range(len(counts)) if counts[j] > 0), key=lambda j: (-int(counts[j]), j))
    out = []
    for j in order:
        c = [float(x) for x in centres[j]]
        rgb = np.array([int(round(x * 255)) for x in colorsys.hsv_to_rgb(c[0] / 255., c[1] / 255., c[2] / 255.)])
        out.append({"cluster_index": j, "HSV_color": c, "RGB_color": rgb, "color_percentage": int(counts[j]) / total})
    return out


def _detect(be, crops, shapes, k, max_iter):
    if k is not None and not 1 <= int(k) <= MAX_K:
        raise ValueError("k must be None or 1 .. %d, got %r" % (MAX_K, k))
    if int(max_iter) < 1:
        raise ValueError("max_iter must be >= 1")
    plan = _plan(shapes)                                  # raises before any entry is called
    results = [None] * len(shapes)
    if not plan["n"]:
        return results
    n = plan["n"]
    hsv = _sample(be, plan, crops)
    centres, counts, passes, dist, labels = _cluster(be, plan, hsv, max_iter)
    dist_h = be.host(dist).view(np.uint64).reshape(n, MAX_K)
    centres_h = be.host(centres).reshape(n, MAX_K, MAX_K, 3)
    counts_h = be.host(counts).view(np.uint32).reshape(n, MAX_K, MAX_K)
    passes_h = be.host(passes).reshape(n, MAX_K)
    distortions = [[int(d) / 65536 / int(plan["points"][i]) for d in dist_h[i]] for i in range(n)]
    ks = [int(k) if k is not None else (opt_k(distortions[i]) or DEFAULT_K) for i in range(n)]
    hist = be.host(_stats(be, plan, ks, hsv, labels)).view(np.uint32).reshape(n, MAX_K, 3, 256)
    patch_crop, low, high = [], [], []
    for i in range(n):
        kk = ks[i]
        clusters = []
        for j in range(kk):
            if counts_h[i, kk - 1, j] == 0:
                continue
            info = {"cluster_index": j}
            info.update(histogram_stats(hist[i, j]))
            info["selected"] = bool(info["Q3"][0] - info["Q1"][0] < H_DIFF)
            clusters.append(info)
            patch_crop.append(i)
            low.append(np.array(np.clip(info["Q1"], 0, 255), dtype=np.uint8))
            high.append(np.array(np.clip(info["Q3"], 0, 255), dtype=np.uint8))
        results[plan["idx"][i]] = {"distortions": distortions[i], "k": kk, "passes": [int(p) for p in passes_h[i]],
                                   "dominant": dominant_colours(centres_h[i, kk - 1, :kk], counts_h[i, kk - 1, :kk]),
                                   "clusters": clusters, "patches": []}
    out, offs = _patches(be, plan, hsv, patch_crop, np.reshape(low, (-1, 3)), np.reshape(high, (-1, 3)))
    for j, i in enumerate(patch_crop):
        dh = int(plan["dst"][i])
        patch = out[int(offs[j]):int(offs[j + 1])]
        results[plan["idx"][i]]["patches"].append(patch.view(dh, WIDTH, 3) if be.device else patch.reshape(dh, WIDTH, 3))
    return results


def detect_headers(crops, k=None, max_iter=300):
    """HeaderDetect.py main() for a batch of table crops on the device.  crops: list of CUDA uint8 (h, w, 3) B,G,R tensors of any
    sizes (what render_detections_device(return_pages=True) and read_images_bgr return; never written).  k: the number of
    clusters, or None for the elbow pick opt_k(distortions), DEFAULT_K when that is None.  max_iter: assignment passes per fit.
    Returns one entry per crop: None for a crop whose sampled height int(h * (500 / w)) is 0, else a dict of
      distortions  the mean distance to the nearest centre for k = 1 .. 9 (plot_elbow_method)
      k            the number of clusters used below
      passes       the assignment passes each of the nine fits took
      dominant     getColorInformation: cluster_index, HSV_color (the centre), RGB_color, color_percentage, by falling count
      clusters     analyse() per non-empty cluster, by index: cluster_index, min_value, max_value, Mean, Std, Q1, Q3, Median, selected
      patches      extractPatches: one CUDA uint8 (dh, 500, 3) B,G,R tensor per entry of clusters
    ValueError, before anything is launched, for a crop whose 500 x dh sampled points exceed 2**21.  The differences from the
    reference are listed in the module docstring."""
    crops = list(crops)
    for i, p in enumerate(crops):
        if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.uint8 and p.dim() == 3 and p.shape[2] == 3
                and p.shape[0] >= 1 and p.shape[1] >= 1):
            raise ValueError("crop %d: a CUDA uint8 (h,w,3) tensor expected, got %s" % (
                i, "%s %s" % (p.dtype, tuple(p.shape)) if isinstance(p, torch.Tensor) else type(p).__name__))
    crops = [p.contiguous() for p in crops]
    return _detect(_Device(crops[0].device) if crops else None, crops, [(p.shape[0], p.shape[1]) for p in crops], k, max_iter)


def detect_headers_twins(crops, k=None, max_iter=300):
    """detect_headers through the CPU twins of the kernels (rtn_header_*_host) over NumPy uint8 (h, w, 3) arrays: the same plan,
    the same host arithmetic, the same results bit for bit with NumPy patches.  For tests and for checking a device result; one
    thread, seconds per crop."""
    crops = [np.ascontiguousarray(p) for p in crops]
    for i, p in enumerate(crops):
        if not (p.dtype == np.uint8 and p.ndim == 3 and p.shape[2] == 3 and p.shape[0] >= 1 and p.shape[1] >= 1):
            raise ValueError("crop %d: a uint8 (h,w,3) array expected, got %s %s" % (i, p.dtype, p.shape))
    return _detect(_Twins(), crops, [p.shape[:2] for p in crops], k, max_iter)


def color_bar(dominant):
    """plotColorBar: the 100 x 500 R,G,B bar of the dominant colours.  cv2.rectangle fills both corner columns, so entry j covers
    the columns int(left) .. int(right) and the next entry paints over the shared one."""
    bar = np.zeros((100, WIDTH, 3), np.uint8)
    top = 0
    for x in dominant:
        bottom = top + x["color_percentage"] * WIDTH
        bar[:, max(int(top), 0):min(int(bottom), WIDTH - 1) + 1] = tuple(int(v) for v in x["RGB_color"])
        top = bottom
    return bar


def header_names(result_dir, crop_name, result):
    """The directory and the file names main() writes for one crop: (directory, [OrigImage.png, colorBar.png, one
    {Selected|Not_Selected}_HSVpatch_<cluster_index>.png per entry of result["clusters"]]); a skipped crop has OrigImage.png alone."""
    d = os.path.join(result_dir, "test_{}".format(os.path.basename(crop_name).split(".")[0]))
    names = [os.path.join(d, "OrigImage.png")]
    if result is not None:
        names.append(os.path.join(d, "colorBar.png"))
        names += [os.path.join(d, "{}_HSVpatch_{}.png".format("Selected" if c["selected"] else "Not_Selected", c["cluster_index"]))
                  for c in result["clusters"]]
    return d, names


def _header_outputs(crops, names, results, result_dir):
    """(paths, images) of a batch in main()'s order; the directories are created."""
    paths, images = [], []
    for crop, name, res in zip(crops, names, results):
        d, files = header_names(result_dir, name, res)
        os.makedirs(d, exist_ok=True)
        paths += files
        images.append(crop)
        if res is not None:
            images.append(np.ascontiguousarray(color_bar(res["dominant"])[:, :, ::-1]))       # imwrite(cvtColor(bar, RGB2BGR))
            images += list(res["patches"])
    return paths, images


def header_files(crop_paths, result_dir, png="host", k=None, max_iter=300, twins=False):
    """The __main__ loop of HeaderDetect.py over crop files: read_images_bgr, detect_headers, one write_images_bgr(..., png=png)
    call for all files of the batch.  Per crop <name>.<ext> it writes result_dir/test_<name>/OrigImage.png, colorBar.png and one
    {Selected|Not_Selected}_HSVpatch_<cluster_index>.png per non-empty cluster (Optimal_K.png and the PDF plot are not written).
    twins=True runs the CPU twins on pages read by read_image_bgr and writes with write_image (no device).  Returns the results."""
    from .page_io import read_image_bgr, read_images_bgr, write_image, write_images_bgr
    crop_paths = list(crop_paths)
    os.makedirs(result_dir, exist_ok=True)
    if twins:
        crops = [read_image_bgr(p) for p in crop_paths]
        results = detect_headers_twins(crops, k=k, max_iter=max_iter)
        for path, image in zip(*_header_outputs(crops, crop_paths, results, result_dir)):
            write_image(path, image)
        return results
    crops = read_images_bgr(crop_paths)
    results = detect_headers(crops, k=k, max_iter=max_iter)
    paths, images = _header_outputs(crops, crop_paths, results, result_dir)
    write_images_bgr(paths, images, png=png)
    return results
