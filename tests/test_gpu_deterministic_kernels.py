"""Deterministic mode, kernel by kernel: every site where several workgroups add floats into one address in arrival order
(colsum, weighted_rowsum, dsmil_attn_bwd, the K-split bag-level gemm_nt, the ATOMIC and WIDE weight-gradient forms), at the smallest
shape that reaches such a form.

Per site: in default mode ``murcl_float_atomic_launches()`` moves across the call (so the shape does reach an arrival-order form);
in the mode it does not move, two calls on the same inputs return the same bits, and the result meets float64 within the tolerance
the existing test of that kernel uses (tests/test_gpu_kernels.py, tests/test_gpu_row_kernels.py - the numbers are copied from there,
the row kernels' checks are imported).  Accumulating variants add into a destination that is not zero."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import murcl_amd  # noqa: E402
from murcl_amd import _lib, ops  # noqa: E402
from tests import test_gpu_row_kernels as RK  # noqa: E402
from tests.test_gpu_kernels import _close, _rand  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _same(a, b):
    a, b = (a if isinstance(a, (tuple, list)) else (a,)), (b if isinstance(b, (tuple, list)) else (b,))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y), f"{int((x != y).sum())}/{x.numel()} elements differ between two calls in deterministic mode"


def _default_then_twice_in_the_mode(call):
    """``call()`` once in default mode (the counter must move) and twice in the mode (it must not; same bits) -> (default, mode)."""
    assert not murcl_amd.is_deterministic()
    c0 = ops.float_atomic_launches()
    default = call()
    assert ops.float_atomic_launches() > c0, "this shape does not reach an arrival-order form in default mode: wrong shape"
    with murcl_amd.deterministic():
        c1 = ops.float_atomic_launches()
        first, second = call(), call()
        assert ops.float_atomic_launches() == c1, "an arrival-order form was launched in deterministic mode"
    assert not murcl_amd.is_deterministic()
    _same(first, second)
    return default, first


# ------------------------------------------------------------------ colsum
@pytest.mark.parametrize("dtype,R,N", [(F32, 2048, 64), (BF16, 2048, 128), (F32, 2048 + 37, 130), (BF16, 600, 72)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_colsum(dtype, R, N, accumulate):
    dev = _dev()
    x = _rand(31, f"x{R}{N}", (R, N)).to(dtype)
    pre = _rand(31, f"p{N}", (N,)) if accumulate else torch.zeros(N)
    xd = x.to(dev)

    def call():
        out = pre.to(dev).clone() if accumulate else torch.full((N,), 3e33, device=dev)      # overwrite: garbage must not survive
        return ops.colsum(xd, out=out, accumulate=accumulate)

    default, det = _default_then_twice_in_the_mode(call)
    ref = pre.double() + x.double().sum(0)
    _close(det, ref, rtol=1e-5, atol=1e-4, msg="colsum in the mode")         # test_cast_transpose_colsum_relu's bound
    _close(default, ref, rtol=1e-5, atol=1e-4, msg="colsum by default")


# ------------------------------------------------------------------ weighted_rowsum (plain and into=), dsmil_attn_bwd
WR_CASES = [(2, 512, 64, 2), (2, 520, 64, 2), (3, 200, 24, 4)]            # 8 even splits; 9 ragged splits of 58 rows; 4 splits, C = 4


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", WR_CASES, ids=lambda c: RK._tag(*c))
def test_weighted_rowsum(case, dtype):
    dev = _dev()
    X, A, _, _, _ = RK.weighted_rowsum_inputs(case, dtype)
    Xd, Ad = X.to(dev), A.to(dev)
    _default_then_twice_in_the_mode(lambda: ops.weighted_rowsum(Xd, Ad))
    with murcl_amd.deterministic():
        RK.check_weighted_rowsum(ops.weighted_rowsum, dev, case, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", WR_CASES[:2], ids=lambda c: RK._tag(*c))
def test_weighted_rowsum_into_adds_to_what_is_there(case, dtype):
    dev = _dev()
    B, N, d, C = case
    X, A, _, ref, _ = RK.weighted_rowsum_inputs(case, dtype)
    Xd, Ad = X.to(dev), A.to(dev)
    pre = RK._n(f"pre{case}", (B, C, d))

    def call():
        return ops.weighted_rowsum(Xd, Ad, into=pre.to(dev).clone())

    _, det = _default_then_twice_in_the_mode(call)
    RK._contract(det, pre.double() + ref, f"weighted_rowsum into a non-zero buffer {case}", larger=("either term", max(pre.abs().max(), ref.abs().max())))
    with murcl_amd.deterministic():
        RK.check_weighted_rowsum_into(ops.weighted_rowsum, dev, case, dtype)


@pytest.mark.parametrize("case", [(2, 70, 3, 136, 4), (2, 64 * 3 + 1, 4, 128, 0)], ids=lambda c: RK._tag(*c))
def test_dsmil_attn_bwd(case):
    dev = _dev()
    B, N, C, ld, q0 = case
    Y, _, qmax, A64, dA = RK.attn_inputs(case)
    args = (A64.float().to(dev), dA.to(dev), Y.to(dev), q0, qmax.to(dev))

    def call():
        dY = torch.full((B * N, ld), RK.SENTINEL, dtype=F32, device=dev)
        return ops.dsmil_attn_bwd(*args, dY, B, N, C), dY

    _default_then_twice_in_the_mode(call)
    with murcl_amd.deterministic():
        RK.check_dsmil_attn_bwd(ops.dsmil_attn_bwd, dev, case)
        # one row block per bag: stored straight to dqmax, no workspace
        RK.check_dsmil_attn_bwd(ops.dsmil_attn_bwd, dev, (2, 1, 3, 136, 4))


def test_dsmil_attn_bwd_without_a_workspace_refuses_in_the_mode():
    dev = _dev()
    B, N, C = 2, 70, 3
    z = torch.zeros((B * N, 128), device=dev)
    a = torch.zeros((B, N, C), device=dev)
    q, dots = torch.zeros((B * C, 128), device=dev), torch.zeros((B * C,), device=dev)
    with murcl_amd.deterministic():
        rc = _lib.lib().murcl_dsmil_attn_bwd(a.data_ptr(), a.data_ptr(), z.data_ptr(), 128, 0, q.data_ptr(), B, N, C, z.data_ptr(), 128,
                                             q.data_ptr(), dots.data_ptr(), _lib.stream())
    assert rc == -1


# ------------------------------------------------------------------ gemm_nt, the K split of the bag-level f32 form
@pytest.mark.parametrize("M,N,K", [(1, 8, 1536), (33, 40, 1536)])         # six 256-k chunks, N no multiple of 16: three K splits
@pytest.mark.parametrize("epi", ["none", "bias_relu", "accumulate"])
def test_gemm_nt_k_split(M, N, K, epi):
    dev = _dev()
    A = _rand(32, f"A{M}{K}", (M, K))
    B = _rand(32, f"B{N}{K}", (N, K), 1 / math.sqrt(K))
    bias, C0 = _rand(32, f"b{N}", (N,)), _rand(32, f"C{M}{N}", (M, N))
    Ad, Bd, bd = A.to(dev), B.to(dev), bias.to(dev)
    ref = A.double() @ B.double().t()
    if epi == "none":
        call = lambda: ops.gemm_nt(Ad, Bd)                                                     # noqa: E731
    elif epi == "bias_relu":
        call, ref = (lambda: ops.gemm_nt(Ad, Bd, epi=ops.EPI_BIAS_RELU, bias=bd)), torch.relu(ref + bias.double())
    else:
        call, ref = (lambda: ops.gemm_nt(Ad, Bd, out=C0.to(dev).clone(), accumulate=True)), C0.double() + ref
    default, det = _default_then_twice_in_the_mode(call)
    _close(det, ref, rtol=2e-5, atol=2e-5, msg=f"gemm_nt {epi} in the mode")     # test_gemm_nt_bag_level_f32_forms' bound
    _close(default, ref, rtol=2e-5, atol=2e-5, msg=f"gemm_nt {epi} by default")


# ------------------------------------------------------------------ gemm_tn: ATOMIC (f32, bf16) and WIDE by default, PARTS in the mode
@pytest.mark.parametrize("dtype,M,N1,N2,kind", [(F32, 1000, 128, 512, _lib.TN_KIND_ATOMIC), (BF16, 4096, 128, 512, _lib.TN_KIND_ATOMIC),
                                                (BF16, 4096, 256, 128, _lib.TN_KIND_WIDE), (BF16, 1000, 136, 72, _lib.TN_KIND_ATOMIC),
                                                (F32, 768 + 5, 520, 132, _lib.TN_KIND_ATOMIC)])
def test_gemm_tn(dtype, M, N1, N2, kind):
    dev = _dev()
    A = _rand(33, f"A{M}{N1}", (M, N1)).to(dtype)
    B = _rand(33, f"B{M}{N2}", (M, N2)).to(dtype)
    pre, W0 = _rand(33, f"p{N1}", (N1,)), _rand(33, f"w{N1}{N2}", (N1, N2))
    Ad, Bd = A.to(dev), B.to(dev)
    probs = [(Ad, Bd, None, None, None, None)]
    assert ops.gemm_tn_plan(probs, _lib.dt(Ad))[1:] == (0, [kind])                 # default mode: as before
    with murcl_amd.deterministic():
        ws, kinds = ops.gemm_tn_plan(probs, _lib.dt(Ad))[1:]
        assert ws > 0 and kinds == [_lib.TN_KIND_PARTS]

    def call():                                                                    # added into a weight and a bias gradient that hold values
        out, cs = W0.to(dev).clone(), pre.to(dev).clone()
        ops.gemm_tn(Ad, Bd, out=out, colsum_into=cs)
        return out, cs, ops.gemm_tn(Ad, Bd)

    default, det = _default_then_twice_in_the_mode(call)
    s, f32 = math.sqrt(M), dtype == F32
    prod = A.double().t() @ B.double()
    for name, (out, cs, fresh) in (("in the mode", det), ("by default", default)):
        # test_gemm_tn_adds_the_bias_gradient_in_the_same_launch's and test_gemm_tn's bounds
        _close(out, W0.double() + prod, rtol=1e-4, atol=1e-4 * s if f32 else 2e-2 * s, msg=f"dW {name}")
        _close(cs, pre.double() + A.double().sum(0), rtol=1e-4, atol=1e-4 * s if f32 else 1e-3 * s, msg=f"db {name}")
        _close(fresh, prod, rtol=1e-4, atol=1e-4 * s if f32 else 2e-2 * s, msg=f"fresh dW {name}")


def test_gemm_tn_column_sum_rows_in_front_of_a_product_take_the_fixed_order_form():
    """colsum_parts with more than 512 partial rows: by default murcl_colsum's split atomics in front of the product; in the mode
    murcl_colsum_det through the call's workspace."""
    dev = _dev()
    M, N1, N2, R = 256, 128, 64, 1500
    A, B, parts = _rand(34, "A", (M, N1)).to(dev), _rand(34, "B", (M, N2)).to(dev), _rand(34, "parts", (R, N1)).to(dev)

    def call():
        out, cs = torch.zeros((N1, N2), device=dev), torch.ones((N1,), device=dev)
        ops.gemm_tn(A, B, out=out, colsum_into=cs, colsum_parts=(parts, R))
        return out, cs

    _, (out, cs) = _default_then_twice_in_the_mode(call)
    _close(cs, 1.0 + parts.double().sum(0), rtol=1e-5, atol=1e-4, msg="db")
    _close(out, A.double().t() @ B.double(), rtol=2e-5, atol=2e-5 * math.sqrt(M), msg="dW")     # test_gemm_tn_bag_level_f32_forms' bound
