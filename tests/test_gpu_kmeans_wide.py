"""K-means at any feature width and up to 64 clusters (murcl_kmeans_step_wide) and the clustering command.

Parity is pinned as in test_gpu_kmeans.py: from the SAME initial centres the device iterations are scikit-learn's Lloyd
iterations (float64 reference).  The start ``X[linspace(0, N-1, K)]`` puts several centres into one blob: the runs take 3-4
iterations and in several cases scikit-learn relocates an empty cluster."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_kmeans import _blobs  # noqa: E402

# (N, d, K, spread)
CASES = [
    (2000, 768, 10, 0.5),       # a width that is not a power of two
    (1500, 2048, 10, 1.0),      # a ResNet-50 feature width
    (997, 384, 7, 2.0),         # N not a multiple of any tile
    (1200, 500, 4, 1.0),        # d % 32 != 0: the padding path
    (3000, 512, 40, 0.5),       # K > 16 at an old width
    (200, 2048, 10, 0.3),       # the GEMM's split-K shape
    (600, 4096, 64, 0.5),       # both caps; some clusters end with 1 row
    (2500, 1280, 32, 1.0),      # wide and many clusters
]


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(N, d, K, spread):
    """(X, init) of a case, read-only: computed once and shared."""
    X, _ = _blobs(103, N, d, K, spread)
    init = X[np.linspace(0, N - 1, K).astype(int)].copy()
    X.setflags(write=False)
    init.setflags(write=False)
    return X, init


@functools.lru_cache(maxsize=None)
def _sklearn(N, d, K, spread):
    from sklearn.cluster import KMeans
    X, init = _case(N, d, K, spread)
    return KMeans(n_clusters=K, init=init.copy(), n_init=1, algorithm="lloyd", max_iter=300, tol=1e-4).fit(X.astype(np.float64))


def _assert_like_scikit_learn(lab, centers, inertia, it, ref, K):
    agree = (lab == ref.labels_).mean()
    print(f"labels agree {agree:.5f}  inertia {inertia:.6g} vs {ref.inertia_:.6g}  "
          f"centres max |diff| {np.abs(centers - ref.cluster_centers_).max():.3g}  iterations {it} vs {ref.n_iter_}")
    assert agree >= 0.999                                             # float32 vs float64 distances: ties only
    assert inertia == pytest.approx(ref.inertia_, rel=2e-4)
    np.testing.assert_allclose(centers, ref.cluster_centers_, rtol=1e-3, atol=1e-3)
    assert it == ref.n_iter_
    assert lab.min() >= 0 and lab.max() < K and len(np.unique(lab)) == K      # nobody stayed empty


@pytest.mark.parametrize("N,d,K,spread", CASES)
def test_lloyd_iterations_equal_scikit_learn_at_any_width(N, d, K, spread):
    from murcl_amd.utils.clustering import lloyd
    X, init = _case(N, d, K, spread)
    ref = _sklearn(N, d, K, spread)
    labels, centers, inertia, it = lloyd(torch.from_numpy(X.copy()).to(_dev()), torch.from_numpy(init.copy()), max_iter=300, tol=1e-4)
    assert tuple(centers.shape) == (K, d) and tuple(labels.shape) == (N,)
    _assert_like_scikit_learn(labels.cpu().numpy(), centers.cpu().numpy(), inertia, it, ref, K)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("N,d,K,spread", [(200, 2048, 10, 0.3), (2000, 768, 10, 0.5)])
def test_runs_are_bit_reproducible_without_float_atomics(N, d, K, spread, det):
    import murcl_amd
    from murcl_amd import ops
    from murcl_amd.utils.clustering import kmeans
    Xd = torch.from_numpy(_case(N, d, K, spread)[0].copy()).to(_dev())
    prev = murcl_amd.set_deterministic(det)
    try:
        before = ops.float_atomic_launches()
        a = kmeans(Xd, K, seed=985)
        b = kmeans(Xd, K, seed=985)
        after = ops.float_atomic_launches()
        assert murcl_amd.is_deterministic() == det                    # the seeding hands the mode back as it found it
    finally:
        murcl_amd.set_deterministic(prev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert after == before
    assert tuple(a[1].shape) == (K, d) and int(a[0].min()) >= 0 and int(a[0].max()) < K


def _hand_loop(entry, ws_query, Xd, init, max_iter=300, tol=1e-4):
    """Lloyd's loop written out on one C-ABI step entry (a start without empty clusters: no relocation)."""
    from murcl_amd._lib import check, ptr, stream
    N, d = Xd.shape
    K = init.shape[0]
    centers = init.to(Xd.device).clone()
    labels = torch.full((N,), -1, dtype=torch.int32, device=Xd.device)
    counts = torch.empty((K,), dtype=torch.int32, device=Xd.device)
    mind2 = torch.empty((N,), dtype=torch.float32, device=Xd.device)
    stats = torch.zeros((3 + K,), dtype=torch.float32, device=Xd.device)
    ws = torch.empty((ws_query(N, d, K) + 3) // 4, dtype=torch.float32, device=Xd.device)
    thresh = tol * float(Xd.var(0, unbiased=False).mean())

    def step(update):
        check(entry(ptr(Xd), N, d, K, ptr(centers), ptr(labels), ptr(counts), ptr(stats), ptr(mind2), update, ptr(ws), stream()), "step")
        return stats.cpu().numpy()

    it = 0
    while it < max_iter:
        h = step(1)
        it += 1
        assert (h[3:] > 0).all() and h[3:].sum() == N and np.array_equal(h[3:], counts.cpu().numpy())
        if h[2] == 0 or float(h[0]) <= thresh:
            break
    h = step(0)
    return labels, centers, float(h[1]), it, mind2


def test_old_shapes_keep_their_kernel_and_the_wide_entry_agrees_with_it():
    from murcl_amd import _lib
    from murcl_amd.utils.clustering import lloyd
    L = _lib.lib()
    N, d, K = 5000, 512, 10
    X, truth = _blobs(103, N, d, K, 0.5)
    init = torch.from_numpy(X[[int(np.nonzero(truth == k)[0][0]) for k in range(K)]].copy())      # one row of every blob
    Xd = torch.from_numpy(X).to(_dev())
    labels, centers, inertia, it = lloyd(Xd, init, max_iter=300, tol=1e-4)
    ol, oc, oi, oit, omd = _hand_loop(L.murcl_kmeans_step, L.murcl_kmeans_workspace_bytes, Xd, init)
    assert torch.equal(labels, ol) and torch.equal(centers, oc) and inertia == oi and it == oit      # bit for bit
    # the wide entry on the same shape: another summation order, so equal to the scikit-learn tolerances, not to the bit
    wl, wc, wi, wit, wmd = _hand_loop(L.murcl_kmeans_step_wide, L.murcl_kmeans_wide_workspace_bytes, Xd, init)
    assert (wl == ol).float().mean().item() >= 0.999
    assert wi == pytest.approx(oi, rel=2e-4) and wit == oit
    np.testing.assert_allclose(wc.cpu().numpy(), oc.cpu().numpy(), rtol=1e-3, atol=1e-3)
    # mind2: squared distance of every row to its centre (|x|^2 ~ 2000 in f32: absolute error ~1e-3 per row)
    np.testing.assert_allclose(wmd.cpu().numpy(), omd.cpu().numpy(), rtol=1e-3, atol=2e-2)
    exact = ((Xd.double() - wc.double()[wl.long()]) ** 2).sum(1)
    np.testing.assert_allclose(wmd.cpu().numpy(), exact.cpu().numpy(), rtol=1e-3, atol=2e-2)


def test_a_width_that_is_no_multiple_of_32_is_padded_with_zero_columns():
    from murcl_amd.utils.clustering import lloyd
    N, d, K, spread = 1200, 500, 4, 1.0
    X, init = _case(N, d, K, spread)
    Xd, initd = torch.from_numpy(X.copy()).to(_dev()), torch.from_numpy(init.copy())
    labels, centers, inertia, it = lloyd(Xd, initd)
    assert tuple(centers.shape) == (K, 500) and centers.is_contiguous()
    pl, pc, pi, pit = lloyd(torch.nn.functional.pad(Xd, (0, 12)).contiguous(), torch.nn.functional.pad(initd, (0, 12)))
    assert tuple(pc.shape) == (K, 512)
    assert torch.equal(labels, pl) and torch.equal(centers, pc[:, :500]) and inertia == pi and it == pit
    assert (pc[:, 500:] == 0).all()


def _parser_spec(parser):
    spec = []
    for a in parser._actions:
        if a.dest == "help":
            continue
        spec.append((a.option_strings[0], a.type, a.default) if a.nargs != 0 else (a.option_strings[0], "store_true"))
    return spec


def test_features_clustering_command(tmp_path, capsys):
    from murcl_amd import features_clustering as FC
    from murcl_amd.utils.datasets import BagPack, select_indices
    assert _parser_spec(FC.build_parser()) == [("--feat_dir", str, ""), ("--num_clusters", int, 10), ("--exist_ok", "store_true")]
    assert FC.build_parser().parse_args([]).exist_ok is False
    rows = {"a": 300, "b": 450, "c": 600, "tiny": 5}
    feats = {}
    for j, (case, n) in enumerate(rows.items()):
        feats[case] = _blobs(200 + j, n, 768, 10, 0.5)[0]
        np.savez(tmp_path / f"{case}.npz", img_features=feats[case])
    FC.main(["--feat_dir", str(tmp_path), "--num_clusters", "10"])
    out = capsys.readouterr().out
    assert "tiny's number of features < number of clusters, can't clustering." in out
    save_dir = tmp_path / "k-means-10"
    assert sorted(os.listdir(save_dir)) == ["a.json", "a.npz", "b.json", "b.npz", "c.json", "c.npz"]
    for case in "abc":
        n = rows[case]
        idx = np.load(save_dir / f"{case}.npz")["features_cluster_indices"]
        assert idx.shape == (n, 1) and np.issubdtype(idx.dtype, np.integer) and idx.min() >= 0 and idx.max() < 10
        lists = json.load(open(save_dir / f"{case}.json"))
        assert len(lists) == 10 and all(l == sorted(l) for l in lists)
        assert sorted(i for l in lists for i in l) == list(range(n))
        assert all(idx[i, 0] == k for k, l in enumerate(lists) for i in l)
    # a second run without --exist_ok rewrites nothing ...
    stamp = {f: os.stat(save_dir / f).st_mtime_ns for f in os.listdir(save_dir)}
    for f in stamp:
        os.utime(save_dir / f, ns=(stamp[f] - 10 ** 10, stamp[f] - 10 ** 10))          # ten seconds back: a rewrite shows at any clock grain
    stamp = {f: os.stat(save_dir / f).st_mtime_ns for f in stamp}
    FC.main(["--feat_dir", str(tmp_path), "--num_clusters", "10"])
    out = capsys.readouterr().out
    assert all(f"{save_dir / (case + '.npz')} is exists!" in out for case in "abc")
    assert {f: os.stat(save_dir / f).st_mtime_ns for f in stamp} == stamp
    # ... and with it every file is written again (the same bits: the run is reproducible)
    before = {case: np.load(save_dir / f"{case}.npz")["features_cluster_indices"] for case in "abc"}
    FC.main(["--feat_dir", str(tmp_path), "--num_clusters", "10", "--exist_ok"])
    assert all(os.stat(save_dir / f).st_mtime_ns > stamp[f] for f in stamp)
    assert all(np.array_equal(np.load(save_dir / f"{case}.npz")["features_cluster_indices"], before[case]) for case in "abc")
    # the json is what the sub-bag sampler consumes
    lists = json.load(open(save_dir / "c.json"))
    pack = BagPack.from_lists([torch.from_numpy(feats["c"]).to(_dev())], [lists])
    ids, cnt = select_indices(pack, torch.full((1, 10), 0.5, device=_dev()), 256)
    c = cnt.item()
    assert 0 < c <= 256 and (ids[0, :c].diff() > 0).all() and 0 <= ids[0, 0].item() and ids[0, c - 1].item() < 600
