"""Record the reference's own optK on a fixed list of distortion vectors -> tests/golden/header_optk.json, the vectors
tests/test_header_ref.py checks model/header.py opt_k against.

    python tools/gen_header_golden.py --reference /path/to/reference

HeaderDetect.py imports cv2, sklearn, scipy, imutils, kneed and matplotlib at module level; optK uses none of them, so the file is
loaded with empty stand-in modules under those names.  Needs a checkout of the reference; the committed JSON holds only the vectors
and the values optK returned."""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = ("cv2", "sklearn", "sklearn.cluster", "sklearn.metrics", "scipy", "scipy.spatial", "scipy.spatial.distance", "imutils",
         "kneed", "matplotlib", "matplotlib.pyplot")


def load_reference(path):
    for name in STUBS:
        if name not in sys.modules:
            mod = types.ModuleType(name)
            mod.__path__ = []
            sys.modules[name] = mod
    sys.modules["sklearn.cluster"].KMeans = None
    sys.modules["sklearn"].metrics = sys.modules["sklearn.metrics"]
    sys.modules["scipy.spatial.distance"].cdist = None
    sys.modules["kneed"].KneeLocator = None
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    spec = importlib.util.spec_from_file_location("reference_header_detect", os.path.join(path, "HeaderDetect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def vectors():
    """Nine distortions each: elbows at every k, flat and rising curves (None), ties, and values that round at the third place."""
    import numpy as np
    out = [[9.0 - i for i in range(9)], [5.0] * 9, [1.0 + 0.1 * i for i in range(9)], [0.0] * 9,
           [112.664, 84.221, 58.953, 24.925, 22.431, 15.933, 13.513, 11.841, 11.107],
           [15.109, 3.532, 1.776, 1.149, 0.612, 0.23, 0.153, 0.142, 0.132],
           [39.078, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
           [10.0, 9.95, 9.9, 9.85, 9.8, 9.75, 9.7, 9.65, 9.6], [10.0, 9.0, 8.04, 7.1, 6.2, 5.3, 4.4, 3.5, 2.6]]
    for elbow in range(2, 9):
        out.append([100.0 - 10.0 * i if i < elbow else 100.0 - 10.0 * (elbow - 1) - 0.5 * (i - elbow + 1) for i in range(9)])
    rng = np.random.default_rng(0)
    for _ in range(24):
        out.append(sorted((float(x) for x in np.round(rng.random(9) * rng.choice([1.0, 30.0, 200.0]), 3)), reverse=True))
    for _ in range(8):
        out.append([float(x) for x in np.round(rng.random(9) * 50.0, 3)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory that holds the reference's HeaderDetect.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "header_optk.json"))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    rows = []
    for v in vectors():
        with contextlib.redirect_stdout(io.StringIO()):          # optK prints its working
            k = ref.optK(list(v))
        rows.append({"distortions": v, "k": k})
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print("%d vectors, %d without a pick -> %s" % (len(rows), sum(r["k"] is None for r in rows), args.out))


if __name__ == "__main__":
    main()
