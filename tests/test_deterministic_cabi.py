"""Deterministic mode, the parts that need no GPU: the new entry points exist in header, library and binding; the switch, its context
manager and the host-side planners (murcl_gemm_tn_plan, the *_workspace queries) behave as include/murcl_amd.h says; default mode
plans exactly what it planned before."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["murcl_set_deterministic", "murcl_deterministic", "murcl_float_atomic_launches", "murcl_colsum_workspace", "murcl_colsum_det",
       "murcl_weighted_rowsum_workspace", "murcl_weighted_rowsum_det", "murcl_dsmil_attn_bwd_workspace", "murcl_dsmil_attn_bwd_det"]


def _tn_plan(dtype, *shapes, cs_rows=0):
    from murcl_amd import _lib
    arr, kinds = (_lib.TnProblem * len(shapes))(), (ctypes.c_int * len(shapes))()
    for g, (M, N1, N2) in enumerate(shapes):
        arr[g] = _lib.TnProblem(None, None, None, ctypes.c_void_p(16) if cs_rows else None, ctypes.c_void_p(16) if cs_rows else None,
                                M, N1, N2, N1, N2, N2, cs_rows, 0, 1.0)
    return _lib.lib().murcl_gemm_tn_plan(arr, len(shapes), dtype, kinds), list(kinds)


def test_new_symbols_are_in_header_library_and_binding():
    from murcl_amd import _lib, build
    src = open(os.path.join(ROOT, "include", "murcl_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(?:int|long)\s+(murcl_\w+)\s*\(", src))
    so = ctypes.CDLL(build.build())
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/murcl_amd.h"
        assert hasattr(so, name), f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    for name in ("murcl_float_atomic_launches", "murcl_colsum_workspace", "murcl_weighted_rowsum_workspace", "murcl_dsmil_attn_bwd_workspace"):
        assert getattr(_lib.lib(), name).restype is ctypes.c_long


def test_switch_and_context_manager_restore_the_previous_state():
    import murcl_amd
    assert murcl_amd.is_deterministic() is False                       # off by default
    with murcl_amd.deterministic():
        assert murcl_amd.is_deterministic()
        with murcl_amd.deterministic(False):
            assert not murcl_amd.is_deterministic()
        assert murcl_amd.is_deterministic()
    assert not murcl_amd.is_deterministic()
    with pytest.raises(KeyError):
        with murcl_amd.deterministic():
            assert murcl_amd.is_deterministic()
            raise KeyError("inside")
    assert not murcl_amd.is_deterministic()                            # restored after an exception
    assert murcl_amd.set_deterministic(True) is False and murcl_amd.is_deterministic()
    assert murcl_amd.set_deterministic(False) is True and not murcl_amd.is_deterministic()


# (dtype, shape, default kind): every ATOMIC / WIDE row of tests/test_cabi.py's plan table
_A, _W, _P = 4, 5, 3
_ORDER_DEPENDENT = [(1, (16383, 512, 512), _W), (1, (8192, 512, 512), _W), (1, (262144, 256, 384), _W), (1, (262144, 4096, 4096), _W),
                    (1, (4096, 128, 512), _A), (1, (4095, 256, 128), _A), (1, (1000, 136, 72), _A), (0, (513, 512, 512), _A),
                    (0, (768, 3072, 512), _A), (1, (4096, 256, 128), _W), (0, (1000, 128, 512), _A), (1, (600, 1024, 1024), _A)]


@pytest.mark.parametrize("dtype,shape,kind", _ORDER_DEPENDENT)
def test_plan_has_no_atomic_or_wide_product_in_the_mode_and_default_plans_are_unchanged(dtype, shape, kind):
    import murcl_amd
    assert _tn_plan(dtype, shape) == (0, [kind])
    with murcl_amd.deterministic():
        ws, kinds = _tn_plan(dtype, shape)
    assert kinds == [_P]
    M, N1, N2 = shape
    tile = (N1 * N2 + N1) * 4
    # a whole number of partial tiles (+ their column sums), at least one, and no more splits than 32-row slabs: every split has rows
    assert ws >= tile and ws % tile == 0 and ws // tile <= (M + 31) // 32
    assert _tn_plan(dtype, shape) == (0, [kind])


def test_plan_in_the_mode_keeps_square_small_and_parts_and_covers_the_column_sum_rows():
    import murcl_amd
    from murcl_amd import _lib
    L = _lib.lib()
    with murcl_amd.deterministic():
        assert _tn_plan(1, (262144, 512, 512)) == (64 * 512 * 512 * 4, [_lib.TN_KIND_SQUARE])
        assert _tn_plan(0, (512, 512, 512)) == (0, [_lib.TN_KIND_SMALL])
        assert _tn_plan(1, (262144, 128, 512)) == (16809984, [_lib.TN_KIND_PARTS])
        # 4096 partial rows of column sums in front of a bag-level product: their fixed-order form needs a workspace of its own
        need = L.murcl_colsum_workspace(4096, 512, _lib.F32)
        assert need > 0 and _tn_plan(0, (512, 512, 512), cs_rows=4096) == (need, [_lib.TN_KIND_SMALL])
    assert _tn_plan(0, (512, 512, 512), cs_rows=4096) == (0, [_lib.TN_KIND_SMALL])


def test_workspace_queries():
    from murcl_amd import _lib
    L = _lib.lib()
    assert L.murcl_colsum_workspace(512, 64, _lib.F32) == 0                      # one split: single writer, nothing to reduce
    assert L.murcl_colsum_workspace(2048, 64, _lib.F32) == 64 * 64 * 4           # 64 splits of 32 rows
    assert L.murcl_colsum_workspace(2048, 130, _lib.BF16) == 64 * 132 * 4        # rows of the workspace padded to 16 bytes
    assert L.murcl_weighted_rowsum_workspace(2, 64, 64, 2) == 0
    assert L.murcl_weighted_rowsum_workspace(2, 512, 64, 2) == 8 * 2 * 2 * 64 * 4
    assert L.murcl_weighted_rowsum_workspace(2, 520, 64, 2) == 9 * 2 * 2 * 64 * 4
    assert L.murcl_dsmil_attn_bwd_workspace(2, 64, 3) == 0
    assert L.murcl_dsmil_attn_bwd_workspace(2, 70, 3) == 2 * 2 * 3 * 128 * 4


def test_ppo_epoch_workspace_covers_its_weight_gradients_in_the_mode():
    """T * B > 512 rollout rows (the entry script's defaults: 6 x 128): the epoch's weight gradients need a PARTS workspace in the
    mode, which murcl_ppo_epoch_workspace adds behind the epoch's own buffers; by default, and for bag-level rollouts, nothing changes."""
    import murcl_amd
    from murcl_amd import _lib
    L = _lib.lib()
    T, B, S, H = 6, 128, 512, 512
    base, small = L.murcl_ppo_epoch_workspace(T, B, S, H), L.murcl_ppo_epoch_workspace(2, 4, S, H)
    R = T * B
    assert base == (R * (2 * 2048 + 2 * H + 15 * H + 2 * H + 17 + 1) + B * H + 6 * H * H + 2048 * H) * 4      # as before
    with murcl_amd.deterministic():
        need, kinds = _tn_plan(0, (R, 2048, S), (R, H, 2048), (R, 3 * H, H), (R - B, 3 * H, H))
        assert kinds == [_P] * 4 and need > 0
        assert L.murcl_ppo_epoch_workspace(T, B, S, H) == base + max(need, L.murcl_colsum_workspace(R, 3 * H, _lib.F32))
        assert L.murcl_ppo_epoch_workspace(2, 4, S, H) == small
    assert L.murcl_ppo_epoch_workspace(T, B, S, H) == base


def test_colsum_entries_return_for_zero_rows():
    from murcl_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    assert L.murcl_colsum(p, p, 0, 64, 64, _lib.F32, 1, None) == 0                 # accumulate: nothing to add, no launch
    assert L.murcl_colsum_det(p, p, 0, 64, 64, _lib.F32, 1, None, 0, None) == 0


def test_det_entries_reject_a_missing_workspace_without_launching():
    from murcl_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    assert L.murcl_colsum_det(p, p, 2048, 64, 64, _lib.F32, 0, None, 0, None) == -1
    assert L.murcl_weighted_rowsum_det(p, p, p, 2, 512, 64, 2, _lib.F32, 0, None, 0, None) == -1
    assert L.murcl_weighted_rowsum_det(p, p, p, 2, 512, 60, 2, _lib.F32, 0, p, 1 << 20, None) == -1     # d % 8
    assert L.murcl_dsmil_attn_bwd_det(p, p, p, 128, 0, p, 2, 70, 3, p, 128, p, p, None, 0, None) == -1
