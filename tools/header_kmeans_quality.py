"""Clustering quality of header detection's k-means chain against the reference's estimator: for every "table"
fixture of tests/header_cases.py and k = 2 .. 9, the float64 inertia of the chain's final labels and centres over the worst and
the best of twenty KMeans(n_clusters=k, random_state=s, n_init=1) fits, s = 0 .. 19.  CPU only; needs sklearn.

    python tools/header_kmeans_quality.py > profiles/header_kmeans_quality.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sklearn  # noqa: E402

import header_cases as K  # noqa: E402
import test_header_ref as T  # noqa: E402


def main():
    print("k-means chain (variance-split start, float32 centres) against sklearn %s KMeans(n_init=1), seeds 0..19" % sklearn.__version__)
    print("H,S,V points by the package's sampler; inertia recomputed in float64 from the final labels and centres")
    print("%-14s %2s %14s %14s %14s %9s %9s" % ("fixture", "k", "ours", "worst start", "best start", "/ worst", "/ best"))
    top_worst = top_best = 0.0
    for name in T.QUALITY_CASES:
        o = K.oracle(name)
        pts = o["hsv"].reshape(-1, 3)
        for k in range(2, 10):
            fit = o["fits"][k - 1]
            ours = T.inertia(pts, fit["labels"], fit["centres"])
            theirs = T.sklearn_inertias(pts, k)
            top_worst, top_best = max(top_worst, ours / max(theirs)), max(top_best, ours / min(theirs))
            print("%-14s %2d %14.6g %14.6g %14.6g %9.4f %9.4f" % (name, k, ours, max(theirs), min(theirs), ours / max(theirs),
                                                                 ours / min(theirs)))
    print("largest ratio to the worst start %.6f (the test's bound: 1 + 1e-6), to the best start %.4f" % (top_worst, top_best))


if __name__ == "__main__":
    main()
