"""The DSMIL row kernels (csrc/dsmil.hip) and the CLAM instance-branch kernels (csrc/clam.hip), each entry point on its own against
a plain float64 reference computed on the CPU from the exact bits the kernel reads (bf16 inputs are rounded first, then widened).

Every case is a ``check_*`` function that takes the implementation as a callable: the tests below hand it the ``murcl_amd.ops``
wrapper, tests/test_host_row_kernel_checks.py hands the same functions a plain torch f32 emulation (all must pass) and defective
emulations (each must fail), which is how the assertions are shown to bite without a GPU.

The contract, per tensor: |got - ref| <= 1e-4 * max|ref| + 1e-4 * |ref| (BASELINE.json north_star; these kernels accumulate in f32,
so bf16-stored inputs get the same bound against float64 of the rounded inputs).  Results that are a difference of two sums of
comparable size (dS, dY, dqmax, dWq) take 1e-4 * max(max|ref|, 0.1 * max|larger term|) as the absolute term, the larger term
evaluated in float64 and named in the message.  A bf16 destination that is added to is held to one bf16 ulp of the reference,
2^-7 |ref|.  Gathered rows, ids, predictions, targets and everything a kernel is documented not to touch are compared bit for bit.

Alignment (ld, qcol0 multiples of 4 floats, d a multiple of 8 resp. 4) is a documented precondition of the 16-byte loads and is
kept in every case; nothing here hands a kernel a bad pointer or an out-of-range index.

clam_inst_fwd, case (2, 70, 520, 32, 8, True): two bags cannot carry eight labels at once, so that case runs four times with the
labels shifted by two, which covers every class.  ``rows_dot_wsum``'s ``out`` is held bit for bit to ``rows_dot``: dsmil.hip walks the
rows the same way in both (four rows in flight, a lane owns 8 consecutive columns per 512-column step) and promises the same sums in
the same order for rows_dot's own two schedules; measured equal at every shape and type below."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detrand  # noqa: E402
from murcl_amd import ops  # noqa: E402

T = torch.from_numpy
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
SEED = 83
SENTINEL = 7.25
Q = 128                                          # DS_Q: the width of DSMIL's query
_NAME = {F32: "f32", BF16: "bf16"}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _close(got, want, rtol, atol, msg=""):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    bad = err > tol
    assert not bad.any(), f"{msg}: {int(bad.sum())}/{bad.numel()} off, max err {err.max():.3e} (ref max {want.abs().max():.3e})"


def _contract(got, ref, msg, larger=None):
    """The f32 contract on one tensor.  ``larger`` = (name, max |.|) of the larger of the two sums ``ref`` is the difference of."""
    ref = ref.detach().double()
    assert got.numel() == ref.numel(), f"{msg}: {tuple(got.shape)} for {tuple(ref.shape)}"
    got = got.detach().double().cpu().reshape(ref.shape)
    top, term = (ref.abs().max().item() if ref.numel() else 0.0), "max|ref|"
    if larger is not None and 0.1 * float(larger[1]) > top:
        top, term = 0.1 * float(larger[1]), f"0.1 max|{larger[0]}|"
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    print(f"{msg}: max err {err:.3e}, absolute term {1e-4 * top:.3e} = 1e-4 {term}")
    _close(got, ref, rtol=1e-4, atol=1e-4 * top, msg=f"{msg} [absolute term: 1e-4 {term}]")


def _exact(got, ref, msg):
    got = got.detach().cpu()
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), f"{msg}: {got.dtype} {tuple(got.shape)} for {ref.dtype} {tuple(ref.shape)}"
    assert torch.equal(got, ref), f"{msg}: {int((got != ref).sum())}/{ref.numel()} elements differ"


def _n(name, shape, dtype=F32, std=1.0):
    """Deterministic normal values, already rounded to ``dtype`` (host): ``.double()`` of the result is what a kernel reads."""
    return T(detrand.normal(SEED, name, shape, std)).to(dtype)


def _crit(name, B, N, C):
    """Critical-instance indices [B,C] int32 holding 0, N-1 and repeats."""
    m = detrand.integers(SEED, name, (B, C), 0, N)
    m[0, 0] = 0
    m[B - 1, C - 1] = N - 1
    if C > 2:
        m[:, 2] = m[:, 0]
    return T(m.astype(np.int32))


def _tag(*a):
    return "-".join(_NAME.get(x, str(x)).replace(" ", "") for x in a)


# ------------------------------------------------------------------ rows_dot / rows_dot_bias
ROWS_DOT_CASES = [(3, 5, 8, 1), (2, 66, 520, 3), (3, 7, 1032, 4), (1, 64, 520, 2), (2, 64, 64, 5)]


@functools.lru_cache(maxsize=None)
def rows_dot_inputs(case, dtype):
    B, N, d, C = case
    return _n(f"rdX{case}", (B, N, d), dtype), _n(f"rdV{case}", (B, C, d)), _n(f"rdb{case}", (C,))


def check_rows_dot(impl, dev, case, dtype, with_bias):
    B, N, d, C = case
    X, V, bias = rows_dot_inputs(case, dtype)
    ref = torch.einsum("bnd,bcd->bnc", X.double(), V.double())
    if with_bias:
        ref = ref + bias.double()
    got = impl(X.to(dev), V.to(dev), bias.to(dev)) if with_bias else impl(X.to(dev), V.to(dev))
    assert got.dtype == F32 and tuple(got.shape) == (B, N, C)
    _contract(got, ref, f"rows_dot{'_bias' if with_bias else ''} {case} {_NAME[dtype]}")


# ------------------------------------------------------------------ weighted_rowsum
WEIGHTED_ROWSUM_CASES = [(2, 1, 8, 1), (3, 67, 24, 3), (2, 300, 520, 4), (1, 130, 2056, 2), (2, 64, 64, 5), (1, 65536, 8, 2)]
WEIGHTED_ROWSUM_INTO_CASES = [(3, 67, 24, 3), (2, 300, 520, 4)]


@functools.lru_cache(maxsize=None)
def weighted_rowsum_inputs(case, dtype):
    B, N, d, C = case
    X, A1, A2 = _n(f"wrX{case}", (B, N, d), dtype), _n(f"wrA{case}", (B, N, C)), _n(f"wrA2{case}", (B, N, C))
    ref = [torch.einsum("bnc,bnd->bcd", A.double(), X.double()) for A in (A1, A2)]
    return X, A1, A2, ref[0], ref[1]


def check_weighted_rowsum(impl, dev, case, dtype):
    B, N, d, C = case
    X, A, _, ref, _ = weighted_rowsum_inputs(case, dtype)
    got = impl(X.to(dev), A.to(dev))
    assert got.dtype == F32 and tuple(got.shape) == (B, C, d)
    _contract(got, ref, f"weighted_rowsum {case} {_NAME[dtype]}")


def check_weighted_rowsum_into(impl, dev, case, dtype):
    """``into=`` adds and does not clear: a zeroed buffer holds the first sum, then the sum of both."""
    B, N, d, C = case
    X, A1, A2, ref1, ref2 = weighted_rowsum_inputs(case, dtype)
    buf = torch.zeros((B, C, d), dtype=F32, device=dev)
    out = impl(X.to(dev), A1.to(dev), into=buf)
    assert out.data_ptr() == buf.data_ptr() and tuple(out.shape) == (B, C, d)
    _contract(buf, ref1, f"weighted_rowsum into (first) {case} {_NAME[dtype]}")
    impl(X.to(dev), A2.to(dev), into=buf)
    _contract(buf, ref1 + ref2, f"weighted_rowsum into (second, added) {case} {_NAME[dtype]}", larger=("either sum", max(ref1.abs().max(), ref2.abs().max())))


# ------------------------------------------------------------------ dsmil_softmax_ / dsmil_softmax_bwd
SOFTMAX_CASES = [(1, 1, 1), (3, 257, 3), (2, 1000, 4)]


@functools.lru_cache(maxsize=None)
def softmax_inputs(case):
    B, N, C = case
    sign = torch.tensor([[1.0 if (b + c) % 2 == 0 else -1.0 for c in range(C)] for b in range(B)])
    S = (_n(f"smS{case}", (B, N, C), std=2.0) + 60.0 * sign[:, None, :]).float()      # a large offset per (bag, class)
    return S, torch.softmax(S.double(), 1), _n(f"smdA{case}", (B, N, C))


def check_dsmil_softmax(impl, dev, case):
    S, ref, _ = softmax_inputs(case)
    buf = S.to(dev).clone()
    got = impl(buf)
    assert got.data_ptr() == buf.data_ptr(), "dsmil_softmax_ works in place"
    _contract(got, ref, f"dsmil_softmax_ {case}")
    off = (got.detach().double().cpu().sum(1) - 1.0).abs().max().item()
    print(f"dsmil_softmax_ {case}: max |sum_n A - 1| {off:.3e}")
    assert off <= 1e-5, f"dsmil_softmax_ {case}: rows of A sum to 1 +- {off:.3e}"


def check_dsmil_softmax_bwd(impl, dev, case):
    _, A64, dA = softmax_inputs(case)
    A = A64.float()                                                  # the bits the kernel reads
    a, da = A.double(), dA.double()
    dots = (a * da).sum(1, keepdim=True)
    larger = max((a * da).abs().max(), (a * dots).abs().max())
    got = impl(A.to(dev), dA.to(dev))
    _contract(got, a * (da - dots), f"dsmil_softmax_bwd dS {case}", larger=("A dA, A sum A dA", larger))


# ------------------------------------------------------------------ dsmil_attn / dsmil_attn_bwd
ATTN_CASES = [(2, 64, 2, 128, 0), (3, 70, 4, 136, 4), (2, 130, 5, 136, 4)]              # (B, N, C, ld, qcol0)
ATTN_BWD_CASES = [(2, 1, 3, 136, 4)] + ATTN_CASES


@functools.lru_cache(maxsize=None)
def attn_inputs(case):
    B, N, C, ld, q0 = case
    Qs = _n(f"atQ{case}", (B * N, Q))
    Y = torch.full((B * N, ld), 1e30, dtype=F32)                     # a kernel that ignores qcol0 or ldq reads these
    Y[:, q0:q0 + Q] = Qs
    qmax = _n(f"atq{case}", (B * C, Q))
    logits = torch.einsum("bnk,bck->bnc", Qs.view(B, N, Q).double(), qmax.view(B, C, Q).double()) / math.sqrt(Q)
    return Y, Qs, qmax, torch.softmax(logits, 1), _n(f"atdA{case}", (B, N, C))


def check_dsmil_attn(impl, dev, case):
    B, N, C, ld, q0 = case
    Y, _, qmax, ref, _ = attn_inputs(case)
    got = impl(Y.to(dev), q0, qmax.to(dev), B, N, C)
    assert got.dtype == F32 and tuple(got.shape) == (B, N, C)
    _contract(got, ref, f"dsmil_attn {case}")


def check_dsmil_attn_bwd(impl, dev, case):
    B, N, C, ld, q0 = case
    Y, Qs, qmax, A64, dA = attn_inputs(case)
    A = A64.float()
    a, da, sc = A.double(), dA.double(), 1.0 / math.sqrt(Q)
    qm, qv = qmax.view(B, C, Q).double(), Qs.view(B, N, Q).double()
    dots = (a * da).sum(1, keepdim=True)
    dS = a * (da - dots)
    dY_ref = torch.einsum("bnc,bck->bnk", dS, qm) * sc
    dY_big = max(torch.einsum("bnc,bck->bnk", t, qm).abs().max() for t in (a * da, a * dots)) * sc
    dq_ref = torch.einsum("bnc,bnk->bck", dS, qv) * sc
    dq_big = max(torch.einsum("bnc,bnk->bck", t, qv).abs().max() for t in (a * da, a * dots)) * sc
    dY = torch.full((B * N, ld), SENTINEL, dtype=F32, device=dev)
    poison = torch.full((B * N, ld), 3e33, dtype=F32, device=dev)    # what a scratch buffer of dY's size is likely to hold next
    del poison
    dqmax = impl(A.to(dev), dA.to(dev), Y.to(dev), q0, qmax.to(dev), dY, B, N, C)
    dY = dY.cpu()
    outside = torch.cat([dY[:, :q0], dY[:, q0 + Q:]], 1)
    _exact(outside, torch.full_like(outside, SENTINEL), f"dsmil_attn_bwd {case}: dY columns outside [qcol0, qcol0+128) keep their bits")
    _contract(dY[:, q0:q0 + Q], dY_ref.reshape(B * N, Q), f"dsmil_attn_bwd dY {case}", larger=("sum_c A dA qmax, sum_c A (sum A dA) qmax", dY_big))
    assert tuple(dqmax.shape) == (B * C, Q)
    _contract(dqmax, dq_ref.reshape(B * C, Q), f"dsmil_attn_bwd dqmax {case}", larger=("sum_n A dA Q, sum_n A (sum A dA) Q", dq_big))


# ------------------------------------------------------------------ gather_rows, dsmil_qv, dsmil_qv_bwd(_cls)
GATHER_CASES = [(2, 9, 3, 136, 4, 128), (3, 50, 4, 40, 8, 24), (2, 7, 3, 530, 10, 515)]   # (B, N, C, ld, col0, width)
QV_CASES = [(2, 9, 4, 1), (3, 50, 260, 3), (2, 33, 1028, 2), (1, 4, 2048, 4)]              # (B, N, d, C)


def check_gather_rows(impl, dev, case, dtype):
    B, N, C, ld, col0, width = case
    src, m = _n(f"gr{case}", (B * N, ld), dtype), _crit(f"grm{case}", B, N, C)
    ref = src.view(B, N, ld)[torch.arange(B)[:, None], m.long(), col0:col0 + width].reshape(B * C, width).contiguous()
    _exact(impl(src.to(dev), m.to(dev), B, C, N, col0, width), ref, f"gather_rows {case} {_NAME[dtype]}")


@functools.lru_cache(maxsize=None)
def qv_inputs(case, dtype):
    B, N, d, C = case
    X, m = _n(f"qvX{case}", (B, N, d), dtype), _crit(f"qvm{case}", B, N, C)
    return X, m, _n(f"qvW{case}", (Q, d), std=d ** -0.5), _n(f"qvb{case}", (Q,))


def check_dsmil_qv(impl, dev, case, dtype):
    B, N, d, C = case
    X, m, wq, bq = qv_inputs(case, dtype)
    xm_ref = X[torch.arange(B)[:, None], m.long()].reshape(B * C, d).float()
    q_ref = xm_ref.double() @ wq.double().t() + bq.double()
    xm, q, v = impl(X.to(dev), m.to(dev), wq.to(dev), bq.to(dev), B, N, C)
    _exact(xm, xm_ref, f"dsmil_qv xm {case} {_NAME[dtype]}")
    _contract(q, q_ref, f"dsmil_qv q {case} {_NAME[dtype]}")
    _contract(v, q_ref @ wq.double(), f"dsmil_qv v {case} {_NAME[dtype]}")


@functools.lru_cache(maxsize=None)
def qv_bwd_inputs(case):
    B, N, d, C = case
    BC = B * C
    R, q, xm, wq = _n(f"qbR{case}", (BC, d)), _n(f"qbq{case}", (BC, Q)), _n(f"qbx{case}", (BC, d)), _n(f"qbW{case}", (Q, d), std=d ** -0.5)
    dq = R.double() @ wq.double().t()
    t1, t2 = q.double().t() @ R.double(), dq.t() @ xm.double()
    return R, q, xm, wq, t1 + t2, max(t1.abs().max(), t2.abs().max()), dq.sum(0)


def check_dsmil_qv_bwd(impl, dev, case):
    R, q, xm, wq, dwq_ref, big, dbq_ref = qv_bwd_inputs(case)
    dwq, dbq = impl(R.to(dev), q.to(dev), xm.to(dev), wq.to(dev))
    _contract(dwq, dwq_ref, f"dsmil_qv_bwd dWq {case}", larger=("q^T R, dq^T xm", big))
    _contract(dbq, dbq_ref, f"dsmil_qv_bwd dbq {case}")


def check_dsmil_qv_bwd_cls(impl, dev, case):
    B, N, d, C = case
    R, q, xm, wq = (t.to(dev) for t in qv_bwd_inputs(case)[:4])
    dcmax, known_w, known_b = _n(f"qcd{case}", (B, C)), _n(f"qcw{case}", (C, d)), _n(f"qcb{case}", (C,))
    sums_w = torch.einsum("bc,bcd->cd", dcmax.double(), xm.cpu().view(B, C, d).double())
    sums_b = dcmax.double().sum(0)
    dwq0, dbq0 = impl(R, q, xm, wq)
    dwc, dbc = torch.full((C, d), 12345.0, dtype=F32, device=dev), torch.full((C,), -777.0, dtype=F32, device=dev)
    dwq1, dbq1 = impl(R, q, xm, wq, dcmax=dcmax.to(dev), dwc=dwc, dbc=dbc, accumulate=False)
    _contract(dwc, sums_w, f"dsmil_qv_bwd_cls dWc, overwritten {case}")
    _contract(dbc, sums_b, f"dsmil_qv_bwd_cls dbc, overwritten {case}")
    dwc, dbc = known_w.to(dev).clone(), known_b.to(dev).clone()
    impl(R, q, xm, wq, dcmax=dcmax.to(dev), dwc=dwc, dbc=dbc, accumulate=True)
    _contract(dwc, known_w.double() + sums_w, f"dsmil_qv_bwd_cls dWc, accumulated {case}", larger=("dWc before, the sums", max(known_w.abs().max(), sums_w.abs().max())))
    _contract(dbc, known_b.double() + sums_b, f"dsmil_qv_bwd_cls dbc, accumulated {case}", larger=("dbc before, the sums", max(known_b.abs().max(), sums_b.abs().max())))
    _exact(dwq1, dwq0.cpu(), f"dsmil_qv_bwd_cls dWq against the plain entry {case}")
    _exact(dbq1, dbq0.cpu(), f"dsmil_qv_bwd_cls dbq against the plain entry {case}")


# ------------------------------------------------------------------ rows_dot_wsum
WSUM_CASES = [(2, 64, 64, 2), (3, 68, 520, 1), (2, 8, 1024, 2), (16, 2048, 16, 2)]        # the last: rows_per_wave = 16
WSUM_NONE_CASES = [(2, 64, 64, 3), (2, 66, 64, 2), (2, 64, 1032, 2)]                    # C = 3, N = 66, d = 1032: the plan says 0


@functools.lru_cache(maxsize=None)
def wsum_inputs(case, dtype):
    B, N, d, C = case
    return _n(f"wsX{case}", (B, N, d), dtype), _n(f"wsV{case}", (B, C, d)), _n(f"wsG{case}", (B, N, C))


def check_rows_dot_wsum(impl, dev, case, dtype, rows_dot=None):
    B, N, d, C = case
    X, V, G = wsum_inputs(case, dtype)
    res = impl(X.to(dev), V.to(dev), G.to(dev))
    assert res is not None, f"rows_dot_wsum {case}: the plan covers this shape"
    out, W = res
    assert tuple(out.shape) == (B, N, C) and tuple(W.shape) == (C, d)
    _contract(out, torch.einsum("bnd,bcd->bnc", X.double(), V.double()), f"rows_dot_wsum out {case} {_NAME[dtype]}")
    _contract(W, torch.einsum("bnc,bnd->cd", G.double(), X.double()), f"rows_dot_wsum W {case} {_NAME[dtype]}")
    if rows_dot is not None:                                         # dsmil.hip: the same sums in the same order as rows_dot's schedules
        _exact(out, rows_dot(X.to(dev), V.to(dev)).cpu(), f"rows_dot_wsum out against rows_dot {case} {_NAME[dtype]}")


def check_rows_dot_wsum_none(impl, dev, case):
    X, V, G = wsum_inputs(case, F32)
    assert impl(X.to(dev), V.to(dev), G.to(dev)) is None, f"rows_dot_wsum {case}: not covered, None before any launch"


# ------------------------------------------------------------------ topk_ids
TOPK_SHAPES = [(3, 1, 1), (2, 40, 8), (2, 300, 32), (2, 4096, 8), (2, 4097, 8), (1, 9000, 32), (2, 9, 8), (2, 40, 32)]   # (B, N, k)
TOPK_KINDS = ["distinct", "ties"]                 # N < 2k, where the two selections overlap: (3, 1, 1), (2, 9, 8), (2, 40, 32)
TOPK_HI, TOPK_LO = (17, 273, 3840, 4096), (5, 261, 3839, 4095)   # tied extremes on both sides of 4096 and on n, n + 256


@functools.lru_cache(maxsize=None)
def topk_inputs(shape, kind):
    """Soft-max-like values: non-negative, no NaN, no -0.0."""
    B, N, k = shape
    if kind == "distinct":
        a = np.stack([(detrand.permutation(SEED, f"tk{shape}{b}", N) + 1).astype(np.float32) / np.float32(N) for b in range(B)])
        assert all(len(np.unique(r)) == N for r in a)
    else:
        a = ((detrand.integers(SEED, f"tk{shape}", (B, N), 0, 5) + 1) * 0.125).astype(np.float32)       # five levels
        if N > 4096:
            a[:, list(TOPK_HI)] = 2.0
            a[:, list(TOPK_LO)] = 0.0
            a[:, N - 1] = 0.0 if N > 4097 else a[:, N - 1]
        if B >= 2:
            a[B - 1, :] = 0.25                                       # the uniform soft-max
    top = np.argsort(-a, axis=1, kind="stable")[:, :k]               # lowest index wins ties
    bot = np.argsort(a, axis=1, kind="stable")[:, :k]
    return T(a), T(np.concatenate([top, bot], 1).astype(np.int32))


def check_topk_ids(impl, dev, shape, kind):
    A, ref = topk_inputs(shape, kind)
    _exact(impl(A.to(dev), shape[2]), ref, f"topk_ids {shape} {kind}")


# ------------------------------------------------------------------ clam_inst_fwd
CLAM_CASES = [(3, 40, 512, 8, 2, True), (3, 40, 512, 8, 2, False), (2, 70, 8, 1, 1, False), (2, 70, 520, 32, 8, True),
              (4, 12, 1024, 8, 3, True)]                             # (B, N, L, k, n_cls, subtyping)


def _clam_targets(lab, c, r, k, subtyping):
    """clam.py: inst_eval (the bag's own class: top-k -> 1, bottom-k -> 0), inst_eval_out (another class, with subtyping:
    top-k -> 0), otherwise not evaluated.  -> (target or -1, number of live rows of the pair's class)."""
    if c == lab:
        return (1 if r < k else 0), 2 * k
    return ((0 if r < k else -1), k) if subtyping else (-1, 0)


def _clam_reference(logits, labels, case):
    """float64, row by row: per-class two-way CE, mean over the class's live rows, ``scale``."""
    B, N, L, k, n_cls, sub = case
    R, O, scale = 2 * k, 2 * n_cls, (1.0 / n_cls if sub else 1.0)
    loss, dl = torch.zeros(B, dtype=torch.float64), torch.zeros(B * R, O, dtype=torch.float64)
    pt = torch.full((2, B, n_cls, R), -1, dtype=torch.int64)
    margin = math.inf
    for b in range(B):
        for c in range(n_cls):
            for r in range(R):
                t, cnt = _clam_targets(int(labels[b]), c, r, k, sub)
                pt[1, b, c, r] = t
                if t < 0:
                    continue
                x0, x1 = logits[b, r, 2 * c].item(), logits[b, r, 2 * c + 1].item()
                mx = max(x0, x1)
                lse = mx + math.log(math.exp(x0 - mx) + math.exp(x1 - mx))
                loss[b] += scale * (lse - (x1 if t else x0)) / cnt
                dl[b * R + r, 2 * c] = (math.exp(x0 - lse) - (t == 0)) / cnt * scale
                dl[b * R + r, 2 * c + 1] = (math.exp(x1 - lse) - (t == 1)) / cnt * scale
                pt[0, b, c, r] = 1 if x1 > x0 else 0
                margin = min(margin, abs(x1 - x0))
    return loss, dl, pt, margin


@functools.lru_cache(maxsize=None)
def clam_inputs(case, dtype, shift):
    """Inputs whose every live pair has |x1 - x0| >= 1e-3 max|logit| in float64 (the first seed that gives that), so that a
    prediction cannot hinge on the last bits of an f32 dot product; the check asserts it again."""
    B, N, L, k, n_cls, sub = case
    labels = (torch.arange(B) + shift) % n_cls
    live = torch.tensor([[[_clam_targets(int(labels[b]), c, r, k, sub)[0] >= 0 for c in range(n_cls)] for r in range(2 * k)] for b in range(B)])
    for seed in range(400):
        h = _n(f"ciH{case}{seed}", (B * N, L), dtype)
        W, bias = _n(f"ciW{case}{seed}", (2 * n_cls, L), std=L ** -0.5), _n(f"cib{case}{seed}", (2 * n_cls,), std=0.5)
        ids = []
        for b in range(B):
            p = detrand.permutation(SEED, f"cii{case}{seed}{b}", N)
            ids.append(p[:2 * k] if N >= 2 * k else np.concatenate([p[:k], p[::-1][:k]]))    # N < 2k: ids repeat
        ids = T(np.stack(ids).astype(np.int32))
        rows = (torch.arange(B)[:, None] * N + ids.long()).reshape(-1)
        logits = (h.double()[rows] @ W.double().t() + bias.double()).view(B, 2 * k, 2 * n_cls)
        x = logits.view(B, 2 * k, n_cls, 2)
        gap = (x[..., 1] - x[..., 0]).abs()[live]
        if gap.numel() == 0 or gap.min() >= 1e-3 * logits.abs().max():
            return h, ids, labels, W, bias, logits
    raise AssertionError(f"clam_inst_fwd {case}: no seed separates every live pair")


def clam_shifts(case):
    B, n_cls = case[0], case[4]
    return range(0, n_cls, B) if B < n_cls else (0,)


def check_clam_inst_fwd(impl, dev, case, dtype):
    B, N, L, k, n_cls, sub = case
    seen = set()
    for shift in clam_shifts(case):
        h, ids, labels, W, bias, logits = clam_inputs(case, dtype, shift)
        loss_ref, dl_ref, pt_ref, margin = _clam_reference(logits, labels, case)
        assert margin >= 1e-3 * logits.abs().max().item(), "precondition: every live pair is separated"
        seen |= set(labels.tolist())
        loss, dl, pt = impl(h.to(dev), ids.to(dev), labels.to(dev), W.to(dev), bias.to(dev), B, N, k, n_cls, sub)
        msg = f"clam_inst_fwd {case} {_NAME[dtype]} labels {labels.tolist()}"
        _exact(pt[1], pt_ref[1], f"{msg}: pt targets")
        _exact(pt[0], pt_ref[0], f"{msg}: pt predictions")
        _contract(loss, loss_ref, f"{msg}: loss")
        _contract(dl, dl_ref, f"{msg}: dl")
    assert seen == set(range(n_cls)), "labels cover every class"


# ------------------------------------------------------------------ take_rows, scatter_add_rows_masked
ROW_D = [8, 520]
ROWS0, NROWS = 37, 19


def check_take_rows(impl, dev, d, dtype):
    src = _n(f"trS{d}", (ROWS0, d), dtype)
    rows = detrand.integers(SEED, f"trr{d}", (NROWS,), 0, ROWS0)
    rows[0], rows[1], rows[2] = 0, ROWS0 - 1, rows[3]
    rows = T(rows)
    _exact(impl(src.to(dev), rows.to(dev)), src[rows].float(), f"take_rows d={d} {_NAME[dtype]}")


def check_scatter_add_rows_masked(impl, dev, d, dtype, write_back):
    dst0, h = _n(f"saD{d}", (ROWS0, d), dtype), _n(f"saH{d}", (ROWS0, d), dtype)
    rows = T(detrand.permutation(SEED, f"sar{d}", ROWS0)[:NROWS].copy())                  # distinct
    g0 = _n(f"saG{d}", (NROWS, d))
    on = h[rows].float() > 0
    dst, g = dst0.to(dev).clone(), g0.to(dev).clone()
    impl(dst, h.to(dev), rows.to(dev), g, write_back=write_back)
    dst, g = dst.cpu(), g.cpu()
    msg = f"scatter_add_rows_masked d={d} {_NAME[dtype]} write_back={write_back}"
    other = torch.ones(ROWS0, dtype=torch.bool)
    other[rows] = False
    _exact(dst[other], dst0[other], f"{msg}: rows not named keep their bits")
    _exact(dst[rows][~on], dst0[rows][~on], f"{msg}: masked-off elements keep their bits")
    total = dst0[rows].double() + torch.where(on, g0.double(), torch.zeros((), dtype=torch.float64))
    if dtype == BF16:
        ref = total.to(BF16).double()                                # rounded to bf16 after the add
        err = (dst[rows].double() - ref).abs()
        print(f"{msg}: max err / |ref| {(err / ref.abs().clamp_min(1e-30)).max().item():.3e}, bound 2^-7")
        assert bool((err <= 2.0 ** -7 * ref.abs()).all()), f"{msg}: more than one bf16 ulp from the reference, max err {err.max():.3e}"
    else:
        _contract(dst[rows], total, msg)
    _exact(g, torch.where(on, g0, torch.zeros(())) if write_back else g0, f"{msg}: g afterwards")


# ------------------------------------------------------------------ cross_entropy, group_mean, mul
CE_CASES = [(8, 2, 8), (130, 5, 65), (96, 32, 1), (40, 3, 10)]                            # (R, C, group)


@functools.lru_cache(maxsize=None)
def ce_inputs(case, all_dead):
    R, C, group = case
    G = R // group
    x = _n(f"ceX{case}", (R, C), std=2.0)
    for r in range(1, R, 4):                                         # exact ties at the maximum: the first one decides
        i, j = r % C, (r + 1) % C
        x[r, i] = x[r, j] = x[r].max() + 1.0
    t = T(detrand.integers(SEED, f"ceT{case}", (R,), 0, C))
    t[::5] = -1
    if G >= 2:
        t[(G - 1) * group:] = -1                                     # a group with no live row
    if all_dead:
        t[:] = -1
    return x, t


def check_cross_entropy(impl, dev, case):
    R, C, group = case
    G = R // group
    for all_dead in ([False] if G >= 2 else [False, True]):          # a single group shows "no live row" in a run of its own
        x, t = ce_inputs(case, all_dead)
        live = t >= 0
        cnt = live.view(G, group).sum(1).double()
        assert bool((t < 0).any()) and bool((cnt == 0).any()) == (G >= 2 or all_dead) and (all_dead or bool((cnt > 0).any()))
        lsm = torch.log_softmax(x.double(), 1)
        rowloss = torch.where(live, -lsm.gather(1, t.clamp_min(0)[:, None])[:, 0], torch.zeros((), dtype=torch.float64))
        inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1), torch.zeros((), dtype=torch.float64))
        loss_ref = rowloss.view(G, group).sum(1) * inv
        onehot = torch.nn.functional.one_hot(t.clamp_min(0), C).double()
        dl_ref = (lsm.exp() - onehot) * (live.double() * inv.repeat_interleave(group))[:, None]
        preds_ref = torch.where(live, T(np.argmax(x.numpy(), 1)), torch.full((), -1, dtype=torch.int64))   # np.argmax: the first maximum
        conf_ref = torch.where(live, lsm.gather(1, t.clamp_min(0)[:, None])[:, 0].exp(), torch.zeros((), dtype=torch.float64))
        three = impl(x.to(dev), t.to(dev), group)
        four = impl(x.to(dev), t.to(dev), group, want_conf=True)
        assert len(three) == 3 and len(four) == 4
        msg = f"cross_entropy {case}{' (all ignored)' if all_dead else ''}"
        for a, b, name in zip(three, four, ("loss", "dl", "preds")):
            _exact(a, b.cpu(), f"{msg}: {name} with and without want_conf")
        loss, dl, preds, conf = four
        _exact(preds, preds_ref, f"{msg}: preds")
        _contract(loss, loss_ref, f"{msg}: loss")
        _contract(dl, dl_ref, f"{msg}: dl")
        _contract(conf, conf_ref, f"{msg}: conf")
        dead = (cnt == 0).repeat_interleave(group)
        _exact(loss.cpu()[cnt == 0], torch.zeros(int((cnt == 0).sum())), f"{msg}: loss of a group with no live row")
        _exact(dl.cpu()[dead], torch.zeros(int(dead.sum()), C), f"{msg}: dl of a group with no live row")
        _exact(conf.cpu()[~live], torch.zeros(int((~live).sum())), f"{msg}: conf of ignored rows")


def check_group_mean(impl, dev):
    groups, group = 5, 300
    x = _n("gm", (groups * group,))
    _contract(impl(x.to(dev), groups, group), x.double().view(groups, group).mean(1), f"group_mean {groups} x {group}")


def check_mul(impl, dev):
    x, k = _n("mulx", (1000,)), _n("mulk", (1000,))
    buf, kd = x.to(dev).clone(), k.to(dev).clone()
    out = impl(buf, kd)
    assert out.data_ptr() == buf.data_ptr(), "mul without out= works in place"
    _contract(out, x.double() * k.double(), "mul 1000")
    _exact(kd, k, "mul: the second factor keeps its bits")
    out2 = torch.full((1000,), SENTINEL, dtype=F32, device=dev)
    impl(x.to(dev).clone(), kd, out=out2)
    _exact(out2, out.cpu(), "mul out=")


# ------------------------------------------------------------------ (check, ops entry, argument tuples): the tests below and the host-only run
def _both(cases, *more):
    out = [(c, dt) for c in cases for dt in DTYPES]
    for m in more:
        out = [a + (x,) for a in out for x in m]
    return out


FAMILIES = {
    "rows_dot": (check_rows_dot, "rows_dot", _both(ROWS_DOT_CASES, (False, True))),
    "weighted_rowsum": (check_weighted_rowsum, "weighted_rowsum", _both(WEIGHTED_ROWSUM_CASES)),
    "weighted_rowsum_into": (check_weighted_rowsum_into, "weighted_rowsum", _both(WEIGHTED_ROWSUM_INTO_CASES)),
    "dsmil_softmax": (check_dsmil_softmax, "dsmil_softmax_", [(c,) for c in SOFTMAX_CASES]),
    "dsmil_softmax_bwd": (check_dsmil_softmax_bwd, "dsmil_softmax_bwd", [(c,) for c in SOFTMAX_CASES]),
    "dsmil_attn": (check_dsmil_attn, "dsmil_attn", [(c,) for c in ATTN_CASES]),
    "dsmil_attn_bwd": (check_dsmil_attn_bwd, "dsmil_attn_bwd", [(c,) for c in ATTN_BWD_CASES]),
    "gather_rows": (check_gather_rows, "gather_rows", _both(GATHER_CASES)),
    "dsmil_qv": (check_dsmil_qv, "dsmil_qv", _both(QV_CASES)),
    "dsmil_qv_bwd": (check_dsmil_qv_bwd, "dsmil_qv_bwd", [(c,) for c in QV_CASES]),
    "dsmil_qv_bwd_cls": (check_dsmil_qv_bwd_cls, "dsmil_qv_bwd", [(c,) for c in QV_CASES]),
    "rows_dot_wsum": (check_rows_dot_wsum, "rows_dot_wsum", _both(WSUM_CASES)),
    "rows_dot_wsum_none": (check_rows_dot_wsum_none, "rows_dot_wsum", [(c,) for c in WSUM_NONE_CASES]),
    "topk_ids": (check_topk_ids, "topk_ids", [(s, kind) for s in TOPK_SHAPES for kind in TOPK_KINDS]),
    "clam_inst_fwd": (check_clam_inst_fwd, "clam_inst_fwd", _both(CLAM_CASES)),
    "take_rows": (check_take_rows, "take_rows", _both(ROW_D)),
    "scatter_add_rows_masked": (check_scatter_add_rows_masked, "scatter_add_rows_masked", _both(ROW_D, (False, True))),
    "cross_entropy": (check_cross_entropy, "cross_entropy", [(c,) for c in CE_CASES]),
    "group_mean": (check_group_mean, "group_mean", [()]),
    "mul": (check_mul, "mul", [()]),
}


def _params(family):
    return pytest.mark.parametrize("args", FAMILIES[family][2], ids=lambda a: _tag(*a) or "one")


def _run(family, args, **kw):
    check, entry, _ = FAMILIES[family]
    check(getattr(ops, entry), _dev(), *args, **kw)


@_params("rows_dot")
def test_rows_dot(args):
    _run("rows_dot", args)


@_params("weighted_rowsum")
def test_weighted_rowsum(args):
    _run("weighted_rowsum", args)


@_params("weighted_rowsum_into")
def test_weighted_rowsum_into_adds_and_does_not_clear(args):
    _run("weighted_rowsum_into", args)


@_params("dsmil_softmax")
def test_dsmil_softmax(args):
    _run("dsmil_softmax", args)


@_params("dsmil_softmax_bwd")
def test_dsmil_softmax_bwd(args):
    _run("dsmil_softmax_bwd", args)


@_params("dsmil_attn")
def test_dsmil_attn(args):
    _run("dsmil_attn", args)


@_params("dsmil_attn_bwd")
def test_dsmil_attn_bwd(args):
    _run("dsmil_attn_bwd", args)


def _attn_bwd_into_garbage(A, dA, Y, qcol0, qmax, dY, B, N, C):
    """``murcl_dsmil_attn_bwd`` as ops.dsmil_attn_bwd calls it, but on a dqmax that holds garbage: the entry clears it."""
    dqmax = torch.full((B * C, qmax.shape[1]), 1e30, dtype=F32, device=Y.device)
    dots = torch.empty((B * C,), dtype=F32, device=Y.device)
    ops.check(ops._lib.lib().murcl_dsmil_attn_bwd(ops.ptr(A), ops.ptr(dA), ops.ptr(Y), Y.stride(0), qcol0, ops.ptr(qmax), B, N, C, ops.ptr(dY),
                                                  dY.stride(0), ops.ptr(dqmax), ops.ptr(dots), ops.stream()), "dsmil_attn_bwd")
    return dqmax


@pytest.mark.parametrize("case", [c for c in ATTN_BWD_CASES if c[2] <= 4], ids=lambda c: _tag(*c))
def test_dsmil_attn_bwd_clears_dqmax(case):
    check_dsmil_attn_bwd(_attn_bwd_into_garbage, _dev(), case)


@_params("gather_rows")
def test_gather_rows(args):
    _run("gather_rows", args)


@_params("dsmil_qv")
def test_dsmil_qv(args):
    _run("dsmil_qv", args)


@_params("dsmil_qv_bwd")
def test_dsmil_qv_bwd(args):
    _run("dsmil_qv_bwd", args)


@_params("dsmil_qv_bwd_cls")
def test_dsmil_qv_bwd_cls(args):
    _run("dsmil_qv_bwd_cls", args)


@_params("rows_dot_wsum")
def test_rows_dot_wsum(args):
    _run("rows_dot_wsum", args, rows_dot=ops.rows_dot)


@_params("rows_dot_wsum_none")
def test_rows_dot_wsum_returns_none_where_the_plan_refuses(args):
    _run("rows_dot_wsum_none", args)


@_params("topk_ids")
def test_topk_ids(args):
    _run("topk_ids", args)


@_params("clam_inst_fwd")
def test_clam_inst_fwd(args):
    _run("clam_inst_fwd", args)


@_params("take_rows")
def test_take_rows(args):
    _run("take_rows", args)


@_params("scatter_add_rows_masked")
def test_scatter_add_rows_masked(args):
    _run("scatter_add_rows_masked", args)


@_params("cross_entropy")
def test_cross_entropy(args):
    _run("cross_entropy", args)


def test_group_mean():
    _run("group_mean", ())


def test_mul():
    _run("mul", ())


# ------------------------------------------------------------------ refusals that return before any launch
def test_dsmil_softmax_refuses_five_classes():
    with pytest.raises(RuntimeError, match="dsmil_softmax"):
        ops.dsmil_softmax_(torch.zeros((2, 8, 5), dtype=F32, device=_dev()))


@pytest.mark.parametrize("N,k", [(64, 33), (8, 9)])
def test_topk_ids_refuses_k_above_32_or_above_N(N, k):
    with pytest.raises(RuntimeError, match="topk_ids"):
        ops.topk_ids(torch.zeros((2, N), dtype=F32, device=_dev()), k)


def test_dsmil_qv_refuses_d_above_its_limit():
    dev, d = _dev(), 2052
    with pytest.raises(RuntimeError, match="dsmil_qv"):
        ops.dsmil_qv(torch.zeros((1, 4, d), dtype=F32, device=dev), torch.zeros((1, 2), dtype=torch.int32, device=dev),
                     torch.zeros((Q, d), dtype=F32, device=dev), torch.zeros((Q,), dtype=F32, device=dev), 1, 4, 2)
