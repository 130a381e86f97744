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


def test_grouped_weight_gradient_plan_runs_on_host():
    """murcl_gemm_tn_grouped_workspace_bytes is pure host arithmetic: the three encoder weight gradients of BASELINE configs[1]
    (262144 rows, 512 x 512 each) share ONE round of 256 workgroups = 12 (product, tile) pairs x 21 row splits, i.e. 21 x 3 MiB
    of partial tiles where three separate launches wrote 3 x 64 MiB; an ineligible member makes the group ineligible (0)."""
    from murcl_amd import _lib
    L = _lib.lib()

    def probs(*shapes):
        arr = (_lib.TnProblem * len(shapes))()
        for g, (M, N1, N2) in enumerate(shapes):
            arr[g] = _lib.TnProblem(None, None, None, None, None, M, N1, N2, N1, N2, N2, 0)
        return arr

    one = L.murcl_gemm_tn_workspace_bytes(262144, 512, 512, _lib.BF16)
    assert one == 64 * 512 * 512 * 4
    # the 128 x 128 kernel's split partials (the attention weight gradient [262144 x 128]^T [. x 512]): a whole number of
    # [128 x 512] tiles + their column sums; one split, the wide kernel, the small f32 kernel and bag-level row counts need none
    parts = L.murcl_gemm_tn_parts_bytes(262144, 128, 512, _lib.BF16)
    assert parts > 0 and parts % ((128 * 512 + 128) * 4) == 0 and L.murcl_gemm_tn_workspace_bytes(262144, 128, 512, _lib.BF16) == 0
    assert L.murcl_gemm_tn_parts_bytes(262144, 512, 512, _lib.BF16) == 0 and L.murcl_gemm_tn_parts_bytes(128, 512, 512, _lib.F32) == 0
    assert L.murcl_gemm_tn_parts_bytes(768, 3072, 512, _lib.F32) == 0 and L.murcl_gemm_tn_parts_bytes(4096, 128, 512, _lib.BF16) == 0
    three = L.murcl_gemm_tn_grouped_workspace_bytes(probs(*[(262144, 512, 512)] * 3), 3, _lib.BF16)
    assert three == 3 * 21 * 512 * 512 * 4
    # unequal row counts: the longer product gets more splits; every split keeps >= 8 slabs of 32 rows
    two = L.murcl_gemm_tn_grouped_workspace_bytes(probs((65536, 512, 512), (262144, 512, 512)), 2, _lib.BF16)
    assert 0 < two <= 64 * 512 * 512 * 4
    assert L.murcl_gemm_tn_grouped_workspace_bytes(probs((262144, 512, 512), (262144, 128, 512)), 2, _lib.BF16) == 0
    assert L.murcl_gemm_tn_grouped_workspace_bytes(probs((262144, 512, 512)), 1, _lib.F32) == 0
    assert L.murcl_gemm_tn_grouped_workspace_bytes(probs(*[(262144, 512, 512)] * 4), 5, _lib.BF16) == 0


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
