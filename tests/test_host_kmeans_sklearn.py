"""Host side of the scikit-learn-stream k-means seeding: the draw schedule leaves numpy's RandomState exactly where scikit-learn's
``_kmeans_plusplus`` leaves it, the restart rule is scikit-learn's, the new C-ABI entries refuse bad shapes without a launch, and the
command's own flags parse.  No GPU is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.kmeans_sklearn_cases import CASES, GOLDEN, RESTARTS_CASE, SEED, key, live_sklearn, make_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["murcl_kmeans_pp_workspace_bytes", "murcl_kmeans_pp", "murcl_kmeans_center_workspace_bytes", "murcl_kmeans_center"]


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


@pytest.mark.parametrize("N,d,K", [(300, 16, 10), (777, 8, 33), (64, 4, 64), (50, 8, 1), (40, 8, 2), (21, 3, 21)])
def test_draw_schedule_consumes_the_stream_like_scikit_learn(N, d, K):
    from sklearn.cluster import kmeans_plusplus
    from murcl_amd.utils.clustering import sklearn_draws
    X = np.random.RandomState(7).standard_normal((N, d)).astype(np.float32)
    theirs, ours = np.random.RandomState(SEED), np.random.RandomState(SEED)
    for _ in range(3):                                               # consecutive restarts continue the stream
        _, indices = kmeans_plusplus(X, K, random_state=theirs)
        first, uniforms = sklearn_draws(ours, N, K)
        assert first == indices[0]
        assert uniforms.shape == (K - 1, 2 + int(np.log(K))) and uniforms.dtype == np.float64
        assert _same_state(theirs, ours)


def test_draw_schedule_is_the_one_fit_consumes():
    """KMeans.fit seeds with the same function on the centred features: after n_init = 3 restarts its RandomState stands where three
    calls of the schedule leave a fresh one (Lloyd takes no draw)."""
    from sklearn.cluster import KMeans
    from murcl_amd.utils.clustering import sklearn_draws
    X = np.random.RandomState(7).standard_normal((200, 12)).astype(np.float32)
    theirs, ours = np.random.RandomState(SEED), np.random.RandomState(SEED)
    KMeans(5, random_state=theirs, n_init=3).fit(X)
    for _ in range(3):
        sklearn_draws(ours, 200, 5)
    assert _same_state(theirs, ours)


def test_same_clustering_rule_is_scikit_learns():
    from sklearn.cluster._k_means_common import _is_same_clustering as theirs
    from murcl_amd.utils.clustering import _is_same_clustering as ours
    r = np.random.RandomState(3)
    a = r.randint(5, size=400).astype(np.int32)
    perm = r.permutation(5).astype(np.int32)
    b = perm[a]
    c = b.copy()
    c[17] = (c[17] + 1) % 5
    merged = np.minimum(a, 3).astype(np.int32)                       # two labels of a fall onto one: still a function of a
    for x, y in [(a, a), (a, b), (b, a), (a, c), (c, a), (a, merged), (merged, a)]:
        assert ours(x, y, 5) == bool(theirs(np.ascontiguousarray(x), np.ascontiguousarray(y), 5))
    assert ours(a, b, 5) and not ours(a, c, 5)


@pytest.mark.parametrize("N,d,K", [(100, 512, 0), (100, 512, 65), (9, 512, 10), (100, 0, 4), (0, 512, 1), (100, -4, 4)])
def test_seeding_refuses_unsupported_shapes_without_launching(N, d, K):
    from murcl_amd import _lib
    L = _lib.lib()
    assert L.murcl_kmeans_pp_workspace_bytes(N, d, K) < 0
    assert L.murcl_kmeans_pp(None, N, d, K, 0, None, None, None, None, None) == -1


def test_seeding_refuses_a_first_row_outside_the_features_and_centring_an_empty_array():
    from murcl_amd import _lib
    L = _lib.lib()
    assert L.murcl_kmeans_pp(None, 100, 512, 10, 100, None, None, None, None, None) == -1
    assert L.murcl_kmeans_pp(None, 100, 512, 10, -1, None, None, None, None, None) == -1
    assert L.murcl_kmeans_center(None, 0, 512, None, None, None, None) == -1
    assert L.murcl_kmeans_center(None, 100, 0, None, None, None, None) == -1
    assert L.murcl_kmeans_center_workspace_bytes(0, 512) < 0


def test_workspace_queries_hold_what_the_launches_write():
    from murcl_amd import _lib
    L = _lib.lib()
    for N, d, K in [(8, 32, 8), (777, 96, 33), (20000, 2048, 10), (100000, 4096, 64)]:
        T = 2 + int(np.log(K))
        b = L.murcl_kmeans_pp_workspace_bytes(N, d, K)
        # candidate distances [T, N] + closest [N] in f32, a share of every candidate's potential per 64 rows in f64
        assert b % 16 == 0 and b >= (T + 1) * N * 4 + T * ((N + 63) // 64) * 8
        assert b <= (T + 1) * N * 4 + T * ((N + 63) // 64) * 8 + 256
        assert L.murcl_kmeans_center_workspace_bytes(N, d) >= d * 8


def test_header_binding_and_exports_agree_for_the_new_names():
    from murcl_amd import _lib, build
    src = open(os.path.join(ROOT, "include", "murcl_amd.h")).read()
    assert src.count("features_clustering.py:10-16") >= 3            # the seeding and the centring cite the reference lines it serves
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(build.build())
    P, I, Lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    for name in NEW:
        m = re.search(r"\b(int|long)\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in include/murcl_amd.h"
        args = [a.strip() for a in m.group(2).split(",")]
        want = [P if ("*" in a or a.startswith("murcl_stream_t")) else I for a in args]
        assert _lib.SIGNATURES[name] == want
        assert hasattr(lib, name)
        assert getattr(_lib.lib(), name).restype == (Lg if m.group(1) == "long" else I)


def test_command_takes_its_own_flags_beside_the_references():
    from murcl_amd import features_clustering as FC
    p = FC.build_parser(own_flags=True)
    acts = [a.option_strings[0] for a in p._actions if a.dest != "help"]
    assert acts == ["--feat_dir", "--num_clusters", "--exist_ok", "--seeding", "--n_init"]
    args = p.parse_args(["--feat_dir", "x"])
    assert (args.seeding, args.n_init) == ("native", None)
    args = p.parse_args(["--feat_dir", "x", "--seeding", "sklearn", "--n_init", "10"])
    assert (args.seeding, args.n_init) == ("sklearn", 10)
    with pytest.raises(SystemExit):
        p.parse_args(["--seeding", "numpy"])


def test_bad_arguments_raise_before_any_launch():
    import torch
    from murcl_amd.utils import clustering as C
    with pytest.raises(ValueError, match="seeding"):
        C.kmeans(torch.zeros(20, 32), 4, seeding="numpy")
    with pytest.raises(ValueError, match="n_init"):
        C.kmeans(torch.zeros(20, 32), 4, seeding="sklearn", n_init=0)
    with pytest.raises(RuntimeError, match="GPU only"):
        C.kmeans(torch.zeros(20, 32), 4, seeding="sklearn")
    with pytest.raises(RuntimeError, match="GPU only"):
        C.kmeans_plusplus_sklearn(torch.zeros(20, 32), 4, SEED)


def test_fixture_is_complete_and_is_what_the_installed_scikit_learn_computes():
    """The recorded values; with scikit-learn >= 1.4 installed (``n_init`` semantics, first centre by ``choice``) also against a live run."""
    g = np.load(GOLDEN)
    assert sorted(g.files) == sorted(["sklearn_version"] + ["idx_" + key(*c) for c in CASES] + ["lab1_" + key(*c) for c in CASES]
                                     + ["lab10_" + key(*RESTARTS_CASE)])
    for case in CASES:
        N, d, K, sep = case
        idx, lab = g["idx_" + key(*case)], g["lab1_" + key(*case)]
        assert idx.shape == (K,) and len(set(idx.tolist())) == K and 0 <= idx.min() and idx.max() < N
        assert lab.shape == (N,) and sorted(set(lab.tolist())) == list(range(K))
    if not live_sklearn():
        return
    from sklearn.cluster import KMeans, kmeans_plusplus
    for case in (CASES[0], CASES[4], CASES[6]):                      # a few seconds of host k-means; the GPU tests compare all live
        N, d, K, sep = case
        X = make_input(*case)
        assert np.array_equal(kmeans_plusplus(X, K, random_state=SEED)[1], g["idx_" + key(*case)])
        assert np.array_equal(KMeans(K, random_state=SEED, n_init=1).fit(X).labels_, g["lab1_" + key(*case)])
