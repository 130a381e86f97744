"""Inputs of the scikit-learn-stream k-means tests (test_gpu_kmeans_sklearn.py, test_host_kmeans_sklearn.py) and of the script that
records their expected values (tools/make_kmeans_sklearn_golden.py -> tests/golden/kmeans_sklearn_stream.npz)."""
import functools
import os

import numpy as np

SEED = 985                                   # the reference's random_state (wsi_processing/features_clustering.py:11)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_sklearn_stream.npz")

# (N, d, K, sep): on every one scikit-learn's float32 and float64 runs agree (indices, labels), which the recording script asserts
CASES = [
    (1000, 512, 10, 3.0),       # the narrow Lloyd kernel
    (3000, 384, 10, 3.0),       # the wide Lloyd kernel
    (2500, 512, 16, 0.0),       # no structure: a long Lloyd run
    (4096, 1024, 10, 0.5),      # weak structure, the widest narrow shape
    (777, 96, 33, 3.0),         # K > 16, five candidates per step, N no multiple of any tile
    (500, 100, 8, 3.0),         # d % 32 != 0 (and % 4 == 0: the vector loads on an unpadded width)
    (8, 32, 8, 3.0),            # N == K: every row ends as a centre
]
RESTARTS_CASE = CASES[0]                     # labels at n_init = 10 are recorded for this one


def key(N, d, K, sep):
    return f"{N}x{d}x{K}"


@functools.lru_cache(maxsize=None)
def make_input(N, d, K, sep):
    """X float32 [N,d], read-only: K blobs ``sep`` apart with unit noise, from numpy.random.RandomState(1)."""
    r = np.random.RandomState(1)
    c = r.standard_normal((K, d)) * sep
    X = (c[r.randint(K, size=N)] + r.standard_normal((N, d))).astype(np.float32)
    X.setflags(write=False)
    return X


def live_sklearn():
    """Is a scikit-learn installed whose KMeans the fixture records (>= 1.4: ``n_init`` semantics, first centre by ``choice``)?"""
    try:
        import sklearn
    except ImportError:
        return False
    return tuple(int(v) for v in sklearn.__version__.split(".")[:2]) >= (1, 4)
