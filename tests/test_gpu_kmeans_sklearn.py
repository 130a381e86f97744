"""``seeding="sklearn"``: the k-means that reproduces scikit-learn's random stream (features_clustering.py:10-16,
``KMeans(n_clusters, random_state=985)``).  Expected values: tests/golden/kmeans_sklearn_stream.npz (recorded by
tools/make_kmeans_sklearn_golden.py on inputs where scikit-learn's float32 and float64 runs agree exactly) and, with scikit-learn >= 1.4
installed, a live run.  Indices and labels are compared with ``==``: no agreement threshold."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.kmeans_sklearn_cases import CASES, GOLDEN, RESTARTS_CASE, SEED, key, live_sklearn, make_input  # noqa: E402


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def _live_fit(case, n_init):
    """A live ``KMeans(K, random_state=985, n_init=n_init)`` on the float32 input, or None without scikit-learn >= 1.4: computed once."""
    if not live_sklearn():
        return None
    from sklearn.cluster import KMeans
    return KMeans(case[2], random_state=SEED, n_init=n_init).fit(make_input(*case))


@functools.lru_cache(maxsize=None)
def _ours(case, n_init):
    """(labels, centers, inertia) of ``kmeans(..., seeding="sklearn")`` as numpy / float: computed once and shared."""
    from murcl_amd.utils.clustering import kmeans
    lab, cent, inertia = kmeans(torch.from_numpy(make_input(*case).copy()).to(_dev()), case[2], seed=SEED, n_init=n_init, seeding="sklearn")
    return lab.cpu().numpy(), cent.cpu().numpy(), inertia


def _inertia_abs(case):
    """4 ulp (f32) of the largest squared row norm of the centred features, per row."""
    X = make_input(*case).astype(np.float64)
    return case[0] * 4 * float(np.finfo(np.float32).eps) * float(((X - X.mean(0)) ** 2).sum(1).max())


@pytest.mark.parametrize("case", CASES, ids=[key(*c) for c in CASES])
def test_seeding_indices_equal_scikit_learns(case):
    from murcl_amd.utils.clustering import kmeans_plusplus_sklearn
    N, d, K, sep = case
    X = make_input(*case)
    Xd = torch.from_numpy(X.copy()).to(_dev())
    centers, indices = kmeans_plusplus_sklearn(Xd, K, SEED)
    print("indices", indices.tolist())
    assert indices.dtype == np.int64 and indices.shape == (K,)
    assert np.array_equal(indices, _golden()["idx_" + key(*case)])
    assert tuple(centers.shape) == (K, d) and np.array_equal(centers.cpu().numpy(), X[indices])      # the centres are those rows
    if live_sklearn():
        from sklearn.cluster import kmeans_plusplus
        assert np.array_equal(indices, kmeans_plusplus(X, K, random_state=SEED)[1])
    # a RandomState is consumed as scikit-learn consumes it: a second seeding from the same state continues the stream
    rs = np.random.RandomState(SEED)
    assert np.array_equal(kmeans_plusplus_sklearn(Xd, K, rs)[1], indices)
    if live_sklearn() and K > 1:
        ref = np.random.RandomState(SEED)
        kmeans_plusplus(X, K, random_state=ref)
        assert np.array_equal(rs.get_state()[1], ref.get_state()[1]) and rs.get_state()[2] == ref.get_state()[2]


@pytest.mark.parametrize("case", CASES, ids=[key(*c) for c in CASES])
def test_labels_equal_scikit_learns_at_one_start(case):
    N, d, K, sep = case
    lab, cent, inertia = _ours(case, 1)
    want = _golden()["lab1_" + key(*case)]
    print(f"labels differing from the fixture: {(lab != want).sum()} of {N}")
    assert lab.shape == (N,) and np.array_equal(lab, want)
    ref = _live_fit(case, 1)
    if ref is not None:
        print(f"inertia {inertia:.7g} vs {ref.inertia_:.7g}  centres max |diff| {np.abs(cent - ref.cluster_centers_).max():.3g}")
        assert np.array_equal(lab, ref.labels_)
        # the tolerances tests/test_gpu_kmeans.py uses for Lloyd against scikit-learn; at N == K the inertia is 0 and only an absolute
        # bound means anything: a row's distance is |x|^2 + (|c|^2 - 2 x.c) in f32, a few ulp of |x|^2 off per row
        assert inertia == pytest.approx(ref.inertia_, rel=2e-4, abs=_inertia_abs(case))
        np.testing.assert_allclose(cent, ref.cluster_centers_, rtol=1e-3, atol=1e-3)


def test_labels_equal_scikit_learns_at_ten_starts():
    """The stream continues across restarts, and a restart of lower inertia but the same partition does not replace the best."""
    case = RESTARTS_CASE
    lab, cent, inertia = _ours(case, 10)
    assert np.array_equal(lab, _golden()["lab10_" + key(*case)])
    ref = _live_fit(case, 10)
    if ref is not None:
        assert np.array_equal(lab, ref.labels_)
        assert inertia == pytest.approx(ref.inertia_, rel=2e-4)
        np.testing.assert_allclose(cent, ref.cluster_centers_, rtol=1e-3, atol=1e-3)


def test_sklearn_mode_defaults_to_one_start_and_clustering_passes_the_mode_on():
    from murcl_amd.utils.clustering import clustering, kmeans
    case = CASES[5]
    X = make_input(*case)
    lab, cent, inertia = kmeans(torch.from_numpy(X.copy()).to(_dev()), case[2], seeding="sklearn")      # seed 985, n_init None -> 1
    assert np.array_equal(lab.cpu().numpy(), _golden()["lab1_" + key(*case)]) and lab.dtype == torch.int32
    idx = clustering(X.copy(), case[2], seeding="sklearn")
    assert idx.shape == (case[0], 1) and idx.dtype == np.int64 and np.array_equal(idx[:, 0], _golden()["lab1_" + key(*case)])


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[5]], ids=[key(*c) for c in (CASES[0], CASES[4], CASES[5])])
def test_runs_are_bit_identical_in_either_mode(case, det):
    import murcl_amd
    from murcl_amd import ops
    from murcl_amd.utils.clustering import kmeans, kmeans_plusplus_sklearn
    Xd = torch.from_numpy(make_input(*case).copy()).to(_dev())
    prev = murcl_amd.set_deterministic(det)
    try:
        before = ops.float_atomic_launches()
        a = kmeans(Xd, case[2], seed=SEED, n_init=1, seeding="sklearn")
        b = kmeans(Xd, case[2], seed=SEED, n_init=1, seeding="sklearn")
        sa, sb = kmeans_plusplus_sklearn(Xd, case[2], SEED), kmeans_plusplus_sklearn(Xd, case[2], SEED)
        after = ops.float_atomic_launches()
        assert murcl_amd.is_deterministic() == det
    finally:
        murcl_amd.set_deterministic(prev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert torch.equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    assert after == before                                            # no float atomics anywhere
    shared = _ours(case, 1)                                           # computed in whichever mode came first: the mode changes no bit
    assert np.array_equal(a[0].cpu().numpy(), shared[0]) and np.array_equal(a[1].cpu().numpy(), shared[1]) and a[2] == shared[2]


def test_centring_is_the_f64_column_mean_rounded_to_f32():
    from murcl_amd.utils.clustering import _center
    for N, d in [(777, 96), (1000, 513), (3, 1), (5000, 300)]:
        X = (np.random.RandomState(2).standard_normal((N, d)) * 3 + 50).astype(np.float32)
        Xc, mean = _center(torch.from_numpy(X).to(_dev()))
        want = X.astype(np.float64).mean(0)
        # the fixed-order f64 sum differs from numpy's pairwise f64 sum by ~1e-16 relative: after rounding to f32 at most one ulp apart
        got = mean.cpu().numpy()
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)))
        assert np.array_equal(Xc.cpu().numpy(), X - got[None, :])


def test_command_with_sklearn_seeding_writes_scikit_learns_partition(tmp_path, capsys):
    from murcl_amd import features_clustering as FC
    cases = {"a": CASES[0], "b": CASES[5]}                            # K = 10 at d = 512 and K = 8 at d = 100: a directory each
    for name, case in cases.items():
        feat_dir = tmp_path / name
        os.makedirs(feat_dir)
        np.savez(feat_dir / "slide.npz", img_features=make_input(*case))
        FC.main(["--feat_dir", str(feat_dir), "--num_clusters", str(case[2]), "--seeding", "sklearn"])
        want = _golden()["lab1_" + key(*case)]
        out = feat_dir / f"k-means-{case[2]}"
        idx = np.load(out / "slide.npz")["features_cluster_indices"]
        assert idx.shape == (case[0], 1) and np.array_equal(idx[:, 0], want)
        lists = json.load(open(out / "slide.json"))
        assert lists == [np.nonzero(want == k)[0].tolist() for k in range(case[2])]
    # --n_init reaches the k-means: ten starts of the first case
    feat_dir = tmp_path / "a"
    FC.main(["--feat_dir", str(feat_dir), "--num_clusters", "10", "--seeding", "sklearn", "--n_init", "10", "--exist_ok"])
    idx = np.load(feat_dir / "k-means-10" / "slide.npz")["features_cluster_indices"]
    assert np.array_equal(idx[:, 0], _golden()["lab10_" + key(*RESTARTS_CASE)])
    capsys.readouterr()


def test_command_without_the_flag_writes_what_clustering_writes(tmp_path, capsys):
    from murcl_amd import features_clustering as FC
    from murcl_amd.utils.clustering import clustering, kmeans, save_to_json
    case = CASES[1]
    X = make_input(*case)
    np.savez(tmp_path / "slide.npz", img_features=X)
    FC.main(["--feat_dir", str(tmp_path), "--num_clusters", "10"])
    capsys.readouterr()
    idx = np.load(tmp_path / "k-means-10" / "slide.npz")["features_cluster_indices"]
    want = clustering(X.copy(), 10)                                   # the default: native seeding, three starts
    assert np.array_equal(idx, want) and idx.dtype == want.dtype
    assert json.load(open(tmp_path / "k-means-10" / "slide.json")) == save_to_json(want, 10)
    # ... which is the native k-means with its defaults spelled out
    lab = kmeans(torch.from_numpy(X.copy()).to(_dev()), 10, seed=985, n_init=3, seeding="native")[0]
    assert np.array_equal(want[:, 0], lab.cpu().numpy())


def test_wrong_arguments_raise_value_error():
    from murcl_amd.utils.clustering import clustering, kmeans, kmeans_plusplus_sklearn
    X = torch.zeros((100, 64), device=_dev())
    with pytest.raises(ValueError):
        kmeans(X, 65, seeding="sklearn")                              # K > 64
    with pytest.raises(ValueError):
        kmeans(X[:9], 10, seeding="sklearn")                          # N < K
    with pytest.raises(ValueError):
        kmeans(X, 10, seeding="scikit")                               # an unknown seeding
    with pytest.raises(ValueError):
        kmeans_plusplus_sklearn(X, 65, SEED)
    with pytest.raises(ValueError):
        kmeans_plusplus_sklearn(X[:9], 10, SEED)
    with pytest.raises(ValueError):
        clustering(np.zeros((100, 64), np.float32), 10, seeding="scikit")


def test_duplicate_rows_and_one_cluster():
    """Fewer distinct rows than clusters: the potential reaches zero and every later draw lands on row 0, as numpy's searchsorted of
    0 into a zero cumulative sum does; K = 1 takes the first draw only."""
    from murcl_amd.utils.clustering import kmeans_plusplus_sklearn
    X = np.repeat(np.random.RandomState(4).standard_normal((3, 40)).astype(np.float32), 5, axis=0)      # 15 rows, 3 distinct
    Xd = torch.from_numpy(X).to(_dev())
    _, indices = kmeans_plusplus_sklearn(Xd, 6, SEED)
    assert len({X[i].tobytes() for i in indices[:3]}) == 3 and indices[3:].tolist() == [0, 0, 0]
    if live_sklearn():
        from sklearn.cluster import kmeans_plusplus
        assert np.array_equal(indices, kmeans_plusplus(X, 6, random_state=SEED)[1])
        assert np.array_equal(kmeans_plusplus_sklearn(Xd, 1, SEED)[1], kmeans_plusplus(X, 1, random_state=SEED)[1])
