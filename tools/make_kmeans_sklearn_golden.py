"""Record what scikit-learn computes on the inputs of tests/kmeans_sklearn_cases.py into tests/golden/kmeans_sklearn_stream.npz:

    python tools/make_kmeans_sklearn_golden.py

per case the k-means++ centre indices (``sklearn.cluster.kmeans_plusplus(X, K, random_state=985)``) and the labels of
``KMeans(K, random_state=985, n_init=1)``; for the first case also the labels at ``n_init=10``.  A case is recorded only if
scikit-learn's float32 and float64 runs agree on it exactly: then differences of rounding size do not move its result, which is the
precision class the device implementation differs by.  Needs scikit-learn >= 1.4 (``n_init`` semantics, first centre by ``choice``)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.kmeans_sklearn_cases import CASES, GOLDEN, RESTARTS_CASE, SEED, key, make_input  # noqa: E402


def record():
    import sklearn
    from sklearn.cluster import KMeans, kmeans_plusplus
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for case in CASES:
        N, d, K, sep = case
        X = make_input(*case)
        idx = {t: kmeans_plusplus(X.astype(t), K, random_state=SEED)[1] for t in (np.float32, np.float64)}
        assert np.array_equal(idx[np.float32], idx[np.float64]), f"{case}: float32 and float64 seedings differ - choose another input"
        out["idx_" + key(*case)] = idx[np.float32].astype(np.int32)
        for n_init in (1, 10) if case == RESTARTS_CASE else (1,):
            fit = {t: KMeans(K, random_state=SEED, n_init=n_init).fit(X.astype(t)) for t in (np.float32, np.float64)}
            assert np.array_equal(fit[np.float32].labels_, fit[np.float64].labels_), f"{case} n_init={n_init}: float32 and float64 labels differ"
            out[f"lab{n_init}_" + key(*case)] = fit[np.float32].labels_.astype(np.int8)
            print(f"{case} n_init={n_init}: {fit[np.float32].n_iter_} iterations, inertia {fit[np.float32].inertia_:.6g}, indices {idx[np.float32].tolist()}")
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    record()
