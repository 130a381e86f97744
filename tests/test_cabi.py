"""The C-ABI library builds, loads without a GPU and exports every symbol include/murcl_amd.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "murcl_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|long)\s+(murcl_\w+)\s*\(", src)))


def test_header_declares_entry_points():
    names = _declared()
    assert "murcl_abmil_pool_fwd" in names and "murcl_ntxent_fwd_bwd" in names and len(names) >= 14


def test_library_builds_and_exports_every_declared_symbol():
    from murcl_amd import build
    lib_path = build.build()
    lib = ctypes.CDLL(lib_path)
    for name in _declared():
        assert hasattr(lib, name), f"{name} declared in include/murcl_amd.h but not exported"


def test_python_binding_covers_header():
    from murcl_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()
    L = _lib.lib()                       # resolves all symbols, sets argtypes; no GPU call
    assert L is _lib.lib()


def test_workspace_queries_run_on_host():
    """Pure host entry points (no launch): chunking of the attention-pool work list, NT-Xent workspace."""
    from murcl_amd import ops, _lib
    for B, N, code, tr in [(128, 2048, _lib.BF16, 32), (4, 256, _lib.F32, 16), (1, 1, _lib.F32, 16), (2, 100000, _lib.BF16, 32)]:
        chunk, S = ops.pool_chunks(B, N, code)
        assert chunk % 16 == 0 and chunk <= 2048 and (S - 1) * chunk < N <= S * chunk
    assert _lib.lib().murcl_ntxent_workspace_bytes(128) >= 128 * 130 * 4


def test_unsupported_arguments_are_rejected_without_launching():
    from murcl_amd import _lib
    L = _lib.lib()
    # K not a multiple of 128 bytes -> -1 before any HIP call
    assert L.murcl_gemm_nt(None, None, None, 8, 8, 30, 30, 30, 8, _lib.F32, _lib.F32, 0, None, None, 0, None, None, 0,
                           None, 0, None) == -1
    assert L.murcl_abmil_pool_fwd(None, None, None, None, None, None, None, None, None, None, 1, 8, 256, 128,
                                  _lib.F32, 1, None) == -1          # L != 512
    assert L.murcl_ntxent_fwd_bwd(None, 7, 128, 1.0, None, None, None, 0, 1, 0, None, None) == -1   # odd n
    assert L.murcl_ntxent_fwd_bwd(None, 24, 128, 1.0, None, None, None, 0, 1, 5, None, None) == -1  # n not a multiple of 2*pair_stride


def _tn_plan(dtype, *shapes, flags=0):
    """murcl_gemm_tn_plan (pure host arithmetic) for products of the given (M, N1, N2) -> (workspace bytes, kinds)."""
    from murcl_amd import _lib
    arr, kinds = (_lib.TnProblem * len(shapes))(), (ctypes.c_int * len(shapes))()
    for g, (M, N1, N2) in enumerate(shapes):
        arr[g] = _lib.TnProblem(None, None, None, None, None, M, N1, N2, N1, N2, N2, 0, flags, 1.0)
    return _lib.lib().murcl_gemm_tn_plan(arr, len(shapes), dtype, kinds), list(kinds)


def test_weight_gradient_plan_query_runs_on_host():
    """murcl_gemm_tn_plan is pure host arithmetic: the three encoder weight gradients of BASELINE configs[1] (262144 rows, 512 x 512
    each) share ONE round of 256 workgroups = 12 (product, tile) pairs x 21 row splits, i.e. 21 x 3 MiB of partial tiles where three
    separate launches wrote 3 x 64 MiB; an ineligible member makes the group run product by product."""
    from murcl_amd import _lib
    SQ = _lib.TN_KIND_SQUARE
    assert _tn_plan(_lib.BF16, (262144, 512, 512)) == (64 * 512 * 512 * 4, [SQ])
    # the 128 x 128 kernel's split partials (the attention weight gradient [262144 x 128]^T [. x 512]): a whole number of
    # [128 x 512] tiles + their column sums; the square tile, the small f32 kernel and bag-level row counts need none
    parts, kinds = _tn_plan(_lib.BF16, (262144, 128, 512))
    assert parts > 0 and parts % ((128 * 512 + 128) * 4) == 0 and kinds == [_lib.TN_KIND_PARTS]
    assert _tn_plan(_lib.F32, (128, 512, 512))[0] == 0 and _tn_plan(_lib.F32, (768, 3072, 512))[0] == 0
    assert _tn_plan(_lib.BF16, (4096, 128, 512))[0] == 0
    three, kinds = _tn_plan(_lib.BF16, *[(262144, 512, 512)] * 3)
    assert three == 3 * 21 * 512 * 512 * 4 and kinds == [SQ] * 3
    # unequal row counts: the longer product gets more splits; every split keeps >= 8 slabs of 32 rows
    two, kinds = _tn_plan(_lib.BF16, (65536, 512, 512), (262144, 512, 512))
    assert 0 < two <= 64 * 512 * 512 * 4 and kinds == [SQ, SQ]
    # not one grouped launch: a member of another kind, f32 tensors, more than four products - product by product, one workspace
    # for all of them (the largest one product needs); flags only on products whose own launch writes C
    mixed, kinds = _tn_plan(_lib.BF16, (262144, 512, 512), (262144, 128, 512))
    assert kinds == [SQ, _lib.TN_KIND_PARTS] and mixed == max(64 * 512 * 512 * 4, parts)
    assert _tn_plan(_lib.BF16, (262144, 512, 512), (262144, 128, 512), flags=_lib.TN_OVERWRITE)[0] < 0
    assert _tn_plan(_lib.F32, (262144, 512, 512))[1] == [_lib.TN_KIND_PARTS]
    five, kinds = _tn_plan(_lib.BF16, *[(262144, 512, 512)] * 5)
    assert five == 64 * 512 * 512 * 4 and kinds == [SQ] * 5
    assert _tn_plan(_lib.BF16, *[(262144, 512, 512)] * 4, (262144, 128, 512), flags=_lib.TN_OVERWRITE)[0] < 0


# (dtype, shapes, flags) -> (workspace bytes, kinds): the dispatch of the weight-gradient products, one row per path and boundary
_S, _Q, _P, _A, _W, _E = 1, 2, 3, 4, 5, 0        # TN_KIND_SMALL, SQUARE, PARTS, ATOMIC, WIDE, EMPTY
_TN_TABLE = [
    (1, [(262144, 512, 512)], 0, 67108864, [_Q]),               # the encoder layers: square tiles
    (1, [(16384, 512, 512)], 0, 67108864, [_Q]),                # fewest rows of the square tiles
    (1, [(16383, 512, 512)], 0, 0, [_W]),                       # one row fewer: the wide kernel
    (1, [(8192, 512, 512)], 0, 0, [_W]),
    (1, [(262144, 256, 384)], 0, 0, [_W]),                      # N2 % 256 == 128: wide at any row count
    (1, [(262144, 4096, 4096)], 0, 0, [_W]),                    # more tiles than an XCD holds: not square
    (1, [(262144, 128, 512)], 0, 16809984, [_P]),               # the attention weight gradient: 64 splits, fixed-order sums
    (1, [(16384, 128, 512)], 0, 16809984, [_P]),
    (1, [(4096, 128, 512)], 0, 0, [_A]),                        # bag-level rows: atomics
    (1, [(4095, 256, 128)], 0, 0, [_A]),                        # one row short of the wide kernel
    (1, [(1000, 136, 72)], 0, 0, [_A]),
    (0, [(512, 512, 512)], 0, 0, [_S]),                         # f32, <= 512 rows: 32 x 32 single-writer tiles
    (0, [(513, 512, 512)], 0, 0, [_A]),
    (0, [(768, 3072, 512)], 0, 0, [_A]),
    (0, [(131072, 128, 1024)], 0, 33587200, [_P]),
    (2, [(131072, 128, 1024)], 0, 16793600, [_P]),              # f32 as a 3-term bf16 split
    (0, [(512, 512, 512)], 1, 0, [_S]),                         # written, not added to
    (0, [(128, 3072, 512), (320, 512, 512)], 0, 0, [_S, _S]),   # a bag-level group: one launch
    (1, [(262144, 512, 512)] * 3, 0, 66060288, [_Q] * 3),       # the encoder group: one launch + one reduce
    (1, [(20000, 512, 512)] * 4, 1, 67108864, [_Q] * 4),
    (0, [(128, 512, 512)], 4, -1, None),                        # a factor the small kernel cannot apply
    (1, [(4096, 128, 512)], 1, -1, None),                       # overwrite needs a launch that writes
    (1, [(0, 512, 512)], 0, 0, [_E]),
    (1, [(4096, 100, 512)], 0, -1, None),                       # N1 not a multiple of 16 bytes
]


@pytest.mark.parametrize("dtype,shapes,flags,ws,kinds", _TN_TABLE)
def test_weight_gradient_plan_table(dtype, shapes, flags, ws, kinds):
    from murcl_amd import _lib
    assert (_lib.TN_KIND_EMPTY, _lib.TN_KIND_SMALL, _lib.TN_KIND_SQUARE, _lib.TN_KIND_PARTS, _lib.TN_KIND_ATOMIC,
            _lib.TN_KIND_WIDE) == (_E, _S, _Q, _P, _A, _W)
    got_ws, got_kinds = _tn_plan(dtype, *shapes, flags=flags)
    if ws < 0:
        assert got_ws < 0
    else:
        assert got_ws == ws and got_kinds == kinds


def test_gate_backward_launcher_returns_for_more_bags_than_partial_rows():
    """with more than 1024 bags the one-pass gate backward's host code looped forever looking for a rows-per-block
    that divides the bag (stage 1 of the contrastive step with CLAM_SB sends 2 T B = 1536 sub-bags).  No GPU is needed to see it
    return: the launch itself fails or succeeds, the planning loop must end."""
    import subprocess
    import sys
    code = ("import ctypes, sys; sys.path.insert(0, %r); from murcl_amd import _lib; L = _lib.lib();"
            "rc = L.murcl_gated_score_bwd_il(None, None, None, None, None, None, None, ctypes.c_void_p(16), 1536 * 1024, 256, _lib.BF16, 0.0, 0, 0,"
            " ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 512, 1024, None); print('returned', rc)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert "returned" in r.stdout, r.stderr[-500:]
