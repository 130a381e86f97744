"""GPU k-means for the clustering pre-step (reference: wsi_processing/features_clustering.py).

``clustering(feats, num_clusters)`` / ``save_to_json(indices, num_clusters)`` keep the reference's signatures and file
formats (``features_cluster_indices`` ``[N,1]`` in an npz; a json list of ``num_clusters`` ascending patch-id lists - the
input of ``WSIWithCluster``).  The reference runs scikit-learn's KMeans(random_state=985) on the host, about a second
per slide; here Lloyd's iterations run on the HIP kernels, without float atomics, so a run is reproducible bit for bit:
``murcl_kmeans_step`` (one pass over the slide's features per iteration) for d in 256 / 512 / 1024 with at most 16 clusters,
``murcl_kmeans_step_wide`` (the same step tiled over d) for every other width - 2048 and 4096 of the reference's ResNet-50 /
VGG-16 extractors, 384 / 768 / 1280 ... - and up to 64 clusters.  Two seedings: ``seeding="native"`` (the default) draws from torch's
generator, so its partitions are not the reference's label for label; what is pinned (tests) is that from the SAME initial centres
the iterations are scikit-learn's Lloyd iterations (same labels, centres and inertia), and that k-means++ seeding + restarts reach
the same inertia range.  ``seeding="sklearn"`` reproduces scikit-learn's stream: the draws of ``_kmeans_plusplus`` come from a host
``numpy.random.RandomState(seed)`` exactly as scikit-learn (>= 1.3) takes them, the arithmetic on the features runs on the device at
scikit-learn's precision (``murcl_kmeans_pp``: f64 sums, f32 distances), X is centred as ``KMeans.fit`` centres it
(``murcl_kmeans_center``) and restarts are kept by scikit-learn's rule.  The partition is then scikit-learn's label for label
WHENEVER no draw lands within rounding distance of a boundary of the cumulative sum and no argmin is a near-tie: scikit-learn adds
its potential in f32 through BLAS, in an order that cannot be copied, so a draw flips with probability of roughly N x (relative
error of that sum); that rate has not been measured at N in the tens of thousands, and the match is no guarantee for every slide.
The line numbers cited below are those of sklearn/cluster/_kmeans.py in scikit-learn 1.7.2.
"""
import json

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream


def _narrow(d, K):
    """Does ``murcl_kmeans_step`` take this shape?  (Those shapes keep that kernel - and their bits.)"""
    return d in (256, 512, 1024) and 1 <= K <= 16


def _step(X, centers, labels, counts, stats, mind2, ws, update):
    N, d = X.shape
    K = centers.shape[0]
    fn, name = ((_lib.lib().murcl_kmeans_step, "kmeans_step") if _narrow(d, K) else
                (_lib.lib().murcl_kmeans_step_wide, "kmeans_step_wide"))
    check(fn(ptr(X), N, d, K, ptr(centers), ptr(labels), ptr(counts), ptr(stats), ptr(mind2), int(update), ptr(ws), stream()), name)


def _relocate_empty(X, centers, labels, mind2, n):
    """scikit-learn's ``_relocate_empty_clusters_dense``: every cluster that received no row is moved onto one of the rows
    farthest from their own centres (largest first), and that row is taken out of the mean of the cluster it was in."""
    empty = np.nonzero(n == 0)[0]
    dist = mind2.cpu().numpy()
    far = np.argpartition(dist, -len(empty))[:-len(empty) - 1:-1]
    n = n.astype(np.float64).copy()
    for e, i in zip(empty, far):
        o = int(labels[i].item())
        x = X[int(i)]
        centers[o] = (centers[o] * n[o] - x) / max(n[o] - 1.0, 1.0)
        n[o] -= 1
        centers[e] = x
        n[e] = 1


def lloyd(X, centers, max_iter=300, tol=1e-4):
    """Lloyd's algorithm from the given centres, with scikit-learn's conventions (what the reference's KMeans call runs):
    stop when no label changes, or when the squared centre shift falls to ``tol * mean feature variance``, or after
    ``max_iter`` iterations; empty clusters are relocated; final labels / inertia are those of the final centres.
    X [N,d] f32 cuda, any d, centers [K,d] with K <= 64.  d in 256/512/1024 with K <= 16 runs on ``murcl_kmeans_step``, every other
    shape on ``murcl_kmeans_step_wide``; a d that is no multiple of 32 is padded once with zero columns (they change no distance
    and no mean) and the returned centres carry the caller's d columns.
    -> (labels int32 [N], centers [K,d], inertia float, iterations)."""
    if not X.is_cuda:
        raise RuntimeError("murcl_amd k-means runs on the GPU only (no CPU fallback)")
    X = X.float().contiguous()
    N, d0 = X.shape
    centers = centers.to(X.device, torch.float32).contiguous().clone()
    K = centers.shape[0]
    if not 1 <= K <= 64 or N < 1 or d0 < 1 or centers.shape[1] != d0:
        raise ValueError(f"k-means takes 1..64 clusters and centres of the features' width (got X {tuple(X.shape)}, centres {tuple(centers.shape)})")
    thresh = tol * float(X.var(0, unbiased=False).mean())             # on the caller's columns: zero pad columns would lower the mean
    if d0 % 32:
        X = torch.nn.functional.pad(X, (0, 32 - d0 % 32)).contiguous()
        centers = torch.nn.functional.pad(centers, (0, 32 - d0 % 32)).contiguous()
    d = X.shape[1]
    labels = torch.full((N,), -1, dtype=torch.int32, device=X.device)
    counts = torch.empty((K,), dtype=torch.int32, device=X.device)
    mind2 = torch.empty((N,), dtype=torch.float32, device=X.device)
    stats = torch.zeros((3 + K,), dtype=torch.float32, device=X.device)
    ws_bytes = (_lib.lib().murcl_kmeans_workspace_bytes if _narrow(d, K) else _lib.lib().murcl_kmeans_wide_workspace_bytes)(N, d, K)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=X.device)
    it = 0
    while it < max_iter:
        prev = centers.clone()
        _step(X, centers, labels, counts, stats, mind2, ws, True)
        it += 1
        h = stats.cpu().numpy()                       # one small copy per iteration steers the loop (an iteration is ~30 us)
        shift = float(h[0])
        if (h[3:] == 0).any():
            _relocate_empty(X, centers, labels, mind2, h[3:])
            shift = float(((centers - prev) ** 2).sum().item())
        if h[2] == 0 or shift <= thresh:              # no label moved (strict convergence), or the centres stopped moving
            break
    _step(X, centers, labels, counts, stats, mind2, ws, False)       # labels and inertia against the final centres
    return labels, (centers[:, :d0].contiguous() if d != d0 else centers), float(stats[1].item()), it


def kmeans_plusplus(X, K, generator):
    """Greedy k-means++ seeding as scikit-learn runs it (``_kmeans_plusplus``: 2 + log K candidate rows per step, drawn
    with probability ~ squared distance to the nearest chosen centre; the candidate that lowers the potential most wins)."""
    N, d = X.shape
    trials = 2 + int(np.log(K))
    if d % 32:                                                # the GEMM's reduction runs in 128-byte slabs: zero columns change no distance
        X = torch.nn.functional.pad(X, (0, 32 - d % 32))
    X = X.contiguous()

    def cross(rows):
        """rows [r, d] . X^T -> [r, N] on the repo's own f32 GEMM (exact-f32 MFMA), not a library matmul: ``murcl_kmeans_cross``, the
        bag-level form of ``ops.gemm_nt`` with its reduction unsplit in either mode (on a small slide of d >= 1536 the default form
        splits it into a zeroed C - float atomics, arrival order - and the seeding must pick the same centres on every run)."""
        rows = rows.contiguous()
        out = torch.empty((rows.shape[0], N), dtype=torch.float32, device=X.device)
        check(_lib.lib().murcl_kmeans_cross(ptr(rows), rows.shape[0], ptr(X), N, X.shape[1], ptr(out), stream()), "kmeans_cross")
        return out

    xx = (X * X).sum(1)
    first = int(torch.randint(N, (1,), generator=generator, device=X.device).item())
    centers = [X[first, :d]]
    d2 = (xx - 2 * cross(X[first:first + 1]).view(-1) + xx[first]).clamp_min_(0)
    for _ in range(1, K):
        pot = d2.sum()
        if float(pot) <= 0:                                   # fewer distinct rows than clusters
            centers.append(X[int(torch.randint(N, (1,), generator=generator, device=X.device).item()), :d])   # (X may carry zero pad columns)
            continue
        cand = torch.multinomial(d2 / pot, trials, replacement=True, generator=generator)
        dc = (xx[None, :] - 2 * cross(X[cand]) + xx[cand][:, None]).clamp_min_(0)         # [trials, N]
        dc = torch.minimum(dc, d2[None, :])
        best = int(dc.sum(1).argmin().item())
        centers.append(X[cand[best], :d])
        d2 = dc[best]
    return torch.stack(centers, 0)


SEEDINGS = ("native", "sklearn")


def sklearn_draws(rs, N, K):
    """The draws scikit-learn's ``_kmeans_plusplus`` takes from ``rs`` (a ``numpy.random.RandomState``) for one seeding of K centres
    among N rows of float32 features, in its order.  -> (row of the first centre, uniforms float64 [K-1, 2 + int(log K)]).
    _kmeans.py:225: the first centre is ``rs.choice(N, p=sample_weight / sample_weight.sum())`` with the float32 unit weights
    ``KMeans.fit`` / ``kmeans_plusplus`` build for float32 features (:1467); :222, :243: every later step draws
    ``rs.uniform(size=2 + int(log K))`` (consecutive doubles of the stream, so one [K-1, trials] draw is the same stream).  Lloyd takes
    no draw, so the seedings of consecutive restarts are consecutive calls.  scikit-learn before 1.3 drew the first centre with
    ``rs.randint(N)``: that variant is not built."""
    w = np.ones(N, dtype=np.float32)
    first = int(rs.choice(N, p=w / w.sum()))
    return first, rs.uniform(size=(K - 1, 2 + int(np.log(K))))


def _check_sklearn_shape(X, K):
    if not X.is_cuda:
        raise RuntimeError("murcl_amd k-means runs on the GPU only (no CPU fallback)")
    if X.dim() != 2 or not 1 <= K <= 64 or X.shape[0] < K or X.shape[1] < 1:
        raise ValueError(f"k-means++ with scikit-learn's stream takes [N,d] features, 1..64 clusters and N >= K (got X {tuple(X.shape)}, K = {K})")


def _seed_sklearn(X, K, first, uniforms):
    """One seeding on the device from the host's draws: K steps enqueued back to back, no host sync. -> (centers [K,d], indices int32 [K], both on the device)."""
    N, d = X.shape
    L = _lib.lib()
    u = torch.from_numpy(np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1)).to(X.device) if K > 1 else None
    indices = torch.empty((K,), dtype=torch.int32, device=X.device)
    centers = torch.empty((K, d), dtype=torch.float32, device=X.device)
    ws = torch.empty(((L.murcl_kmeans_pp_workspace_bytes(N, d, K) + 15) // 16, 2), dtype=torch.float64, device=X.device)
    check(L.murcl_kmeans_pp(ptr(X), N, d, K, first, ptr(u), ptr(indices), ptr(centers), ptr(ws), stream()), "kmeans_pp")
    return centers, indices


def kmeans_plusplus_sklearn(X, K, seed):
    """``sklearn.cluster.kmeans_plusplus(X, K, random_state=seed)`` (scikit-learn >= 1.3) on the device: X [N,d] f32 cuda as given (not
    centred, like that function), ``seed`` an int or a ``numpy.random.RandomState`` (left where scikit-learn would leave it).
    -> (centers [K,d] on the device, indices int64 numpy [K]); the indices are read back once, after the last step."""
    X = X.float().contiguous()
    _check_sklearn_shape(X, K)
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    centers, indices = _seed_sklearn(X, K, *sklearn_draws(rs, X.shape[0], K))
    return centers, indices.cpu().numpy().astype(np.int64)


def _center(X):
    """_kmeans.py:1477-1481: -> (X - column mean, column mean), on the device (mean in f64, rounded to f32)."""
    N, d = X.shape
    L = _lib.lib()
    Xc, mean = torch.empty_like(X), torch.empty((d,), dtype=torch.float32, device=X.device)
    ws = torch.empty(((L.murcl_kmeans_center_workspace_bytes(N, d) + 7) // 8,), dtype=torch.float64, device=X.device)
    check(L.murcl_kmeans_center(ptr(X), N, d, ptr(Xc), ptr(mean), ptr(ws), stream()), "kmeans_center")
    return Xc, mean


def _is_same_clustering(a, b, K):
    """_k_means_common.pyx:314-328: is every label of ``a`` mapped onto one label of ``b``?"""
    pairs = np.unique(a.astype(np.int64) * K + b.astype(np.int64))
    return len(np.unique(pairs // K)) == len(pairs)


def _kmeans_sklearn(X, K, seed, n_init, max_iter, tol):
    """``KMeans(K, random_state=seed, n_init=n_init).fit(X)`` (_kmeans.py:1466-1553): centre, then per restart seed and iterate; a later
    restart replaces the best only if its inertia is strictly lower and its partition differs up to relabelling (:1525-1528)."""
    _check_sklearn_shape(X, K)
    rs = np.random.RandomState(seed)
    draws = [sklearn_draws(rs, X.shape[0], K) for _ in range(n_init)]          # Lloyd takes no draw: all restarts up front, in order
    Xc, mean = _center(X)
    best = best_lab = None
    for first, uniforms in draws:
        out = lloyd(Xc, _seed_sklearn(Xc, K, first, uniforms)[0], max_iter, tol)
        lab = out[0].cpu().numpy()
        if best is None or (out[2] < best[2] and not _is_same_clustering(lab, best_lab, K)):
            best, best_lab = out, lab
    return best[0], best[1] + mean, best[2]


def kmeans(X, num_clusters, seed=985, n_init=None, max_iter=300, tol=1e-4, seeding="native"):
    """Best of ``n_init`` k-means++ starts by inertia.  -> (labels int32 [N], centers, inertia).
    ``seeding="native"`` (default; ``n_init`` defaults to 3) draws from torch's generator.  ``seeding="sklearn"`` reproduces
    ``KMeans(num_clusters, random_state=seed, n_init=n_init)`` of scikit-learn >= 1.3 (see the module docstring for the limit of that
    claim); there ``n_init`` defaults to 1, what ``n_init='auto'`` means for k-means++ (_kmeans.py:879-881) - a run of the reference
    made with an older scikit-learn is reproduced with ``n_init=10``."""
    if seeding not in SEEDINGS:
        raise ValueError(f"seeding is one of {SEEDINGS}, got {seeding!r}")
    if n_init is None:
        n_init = 3 if seeding == "native" else 1
    if n_init < 1:
        raise ValueError(f"n_init >= 1, got {n_init}")
    X = X.float().contiguous()
    if seeding == "sklearn":
        return _kmeans_sklearn(X, num_clusters, seed, n_init, max_iter, tol)
    g = torch.Generator(device=X.device)
    g.manual_seed(seed)
    best = None
    for _ in range(n_init):
        out = lloyd(X, kmeans_plusplus(X, num_clusters, g), max_iter, tol)
        if best is None or out[2] < best[2]:
            best = out
    return best[0], best[1], best[2]


def clustering(feats, num_clusters, filepath=None, device="cuda", seed=985, seeding="native", n_init=None):
    """features_clustering.py:10-16: -> ``features_cluster_indices`` int array [N,1]; saved to ``filepath`` (npz) if given.
    ``seeding="sklearn"``: the partition of the reference's ``KMeans(num_clusters, random_state=seed)`` (see ``kmeans``)."""
    X = torch.as_tensor(np.asarray(feats, dtype=np.float32)) if not isinstance(feats, torch.Tensor) else feats
    labels, _, _ = kmeans(X.to(device), num_clusters, seed=seed, n_init=n_init, seeding=seeding)
    idx = labels.cpu().numpy().astype(np.int64).reshape(-1, 1)
    if filepath is not None:
        np.savez(file=filepath, features_cluster_indices=idx)
    return idx


def save_to_json(features_cluster_indices, num_clusters, filepath=None):
    """features_clustering.py:19-25: ``num_clusters`` ascending patch-id lists (the ``clusters_json_filepath`` format)."""
    lab = np.asarray(features_cluster_indices).reshape(-1)
    lists = [np.nonzero(lab == k)[0].tolist() for k in range(num_clusters)]
    if filepath is not None:
        with open(filepath, "w") as f:
            json.dump(lists, f)
    return lists
