"""Host side of the wide k-means entry: refusals without a launch, the workspace query, header / binding / export agreement,
and the clustering command's parser and CPU refusal.  No GPU is touched."""
import argparse
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["murcl_kmeans_step_wide", "murcl_kmeans_wide_workspace_bytes", "murcl_kmeans_cross"]


@pytest.mark.parametrize("N,d,K", [(100, 500, 4), (100, 0, 4), (100, 512, 0), (100, 512, 65), (0, 512, 4), (100, -32, 4), (100, 2048, -1)])
def test_wide_step_refuses_unsupported_shapes_without_launching(N, d, K):
    from murcl_amd import _lib
    L = _lib.lib()
    assert L.murcl_kmeans_step_wide(None, N, d, K, None, None, None, None, None, 1, None, None) == -1
    assert L.murcl_kmeans_wide_workspace_bytes(N, d, K) < 0


@pytest.mark.parametrize("R,N,d", [(0, 100, 512), (1025, 100, 512), (4, 0, 512), (4, 100, 500), (4, 100, 0)])
def test_cross_terms_refuse_unsupported_shapes_without_launching(R, N, d):
    from murcl_amd import _lib
    assert _lib.lib().murcl_kmeans_cross(None, R, None, N, d, None, None) == -1


def test_wide_workspace_query_is_positive_and_grows_with_the_rows():
    from murcl_amd import _lib
    L = _lib.lib()
    last = 0
    for N in (1, 63, 64, 65, 1000, 20000, 100000, 1000000):
        b = L.murcl_kmeans_wide_workspace_bytes(N, 2048, 10)
        assert b > last and b % 16 == 0
        last = b
    # it holds at least the cross terms [K, N], a row norm per row and one [K, d] partial sum
    for N, d, K in [(200, 2048, 10), (600, 4096, 64), (20000, 32, 1), (3000, 512, 40)]:
        assert L.murcl_kmeans_wide_workspace_bytes(N, d, K) >= (K * N + N + K * d) * 4
    # the row parts' partial sums stay within 32 MiB however wide the features are (as do the 32 folds of the reduction)
    N, d, K = 20000, 4096, 64
    assert L.murcl_kmeans_wide_workspace_bytes(N, d, K) < 2 * (32 << 20) + (K * d + K * N + N) * 4 + (1 << 20)


def test_header_binding_and_exports_agree_for_the_new_names():
    from murcl_amd import _lib, build
    src = open(os.path.join(ROOT, "include", "murcl_amd.h")).read()
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
    # the wide step takes murcl_kmeans_step's arguments, one for one
    assert _lib.SIGNATURES["murcl_kmeans_step_wide"] == _lib.SIGNATURES["murcl_kmeans_step"]
    assert _lib.SIGNATURES["murcl_kmeans_wide_workspace_bytes"] == _lib.SIGNATURES["murcl_kmeans_workspace_bytes"]


def test_routing_keeps_the_old_kernel_for_every_shape_it_takes():
    from murcl_amd.utils import clustering as C
    assert all(C._narrow(d, K) for d in (256, 512, 1024) for K in (1, 10, 16))
    assert not any(C._narrow(d, K) for d, K in [(512, 17), (2048, 10), (768, 10), (384, 7), (4096, 64), (32, 1)])


def test_command_parser_and_cpu_refusal(tmp_path):
    from murcl_amd import features_clustering as FC
    p = FC.build_parser()
    acts = {a.option_strings[0]: a for a in p._actions if a.dest != "help"}
    assert list(acts) == ["--feat_dir", "--num_clusters", "--exist_ok"]
    assert (acts["--feat_dir"].type, acts["--feat_dir"].default) == (str, "")
    assert (acts["--num_clusters"].type, acts["--num_clusters"].default) == (int, 10)
    assert isinstance(acts["--exist_ok"], argparse._StoreTrueAction) and acts["--exist_ok"].default is False
    args = p.parse_args(["--feat_dir", str(tmp_path), "--num_clusters", "12", "--exist_ok"])
    assert (args.feat_dir, args.num_clusters, args.exist_ok) == (str(tmp_path), 12, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        FC.run(args, device="cpu")
    assert not (tmp_path / "k-means-12").exists()                     # refused before anything is written
