"""Host only: the checks of tests/test_gpu_row_kernels.py bite.

Every ``check_*`` there takes the implementation as a callable.  Here each runs on the CPU against a plain torch f32 emulation of
the operation (all must pass: the float64 references and the preconditions are self-consistent), and against emulations with one
defect each, of the kind a kernel rewrite produces (each must fail its check).  Nothing here opens the device."""
import math

import pytest
import torch

import test_gpu_row_kernels as K

CPU = torch.device("cpu")
F32, BF16 = torch.float32, torch.bfloat16


# ------------------------------------------------------------------ the emulations: ops.* signatures, torch f32 on the CPU
def rows_dot(X, V, bias=None, *, drop_last=False):
    out = torch.einsum("bnd,bcd->bnc", X.float(), V)
    if bias is not None:
        out = out + bias
    if drop_last:
        out[:, -1] = 0.0
    return out


def weighted_rowsum(X, A, into=None, *, drop_last=False, clears=False):
    B, N, d = X.shape
    if drop_last:
        X, A = X[:, :-1], A[:, :-1]
    Z = torch.einsum("bnc,bnd->bcd", A, X.float())
    if into is None:
        return Z
    into = into.view(B, -1, d)
    (into.copy_ if clears else into.add_)(Z)
    return into


def dsmil_softmax_(S):
    if S.shape[2] > 4:
        raise RuntimeError("dsmil_softmax")
    return S.copy_(torch.softmax(S, 1))


def dsmil_softmax_bwd(A, dA):
    return A * (dA - (A * dA).sum(1, keepdim=True))


def dsmil_attn(Y, qcol0, qmax, B, N, C, *, scale=1.0 / math.sqrt(K.Q), use_qcol0=True):
    q0 = qcol0 if use_qcol0 else 0
    return torch.softmax(torch.einsum("bnk,bck->bnc", Y[:, q0:q0 + K.Q].reshape(B, N, K.Q), qmax.view(B, C, K.Q)) * scale, 1)


def dsmil_attn_bwd(A, dA, Y, qcol0, qmax, dY, B, N, C, *, dq_rows=None, whole_rows=False):
    sc = 1.0 / math.sqrt(K.Q)
    dS = dsmil_softmax_bwd(A, dA)
    g = (torch.einsum("bnc,bck->bnk", dS, qmax.view(B, C, K.Q)) * sc).reshape(B * N, K.Q)
    if whole_rows:                                                   # the class-group wrapper that added whole scratch rows
        dY += 1.0
        dY[:, qcol0:qcol0 + K.Q] -= 1.0
    dY[:, qcol0:qcol0 + K.Q] = g
    Qv = Y[:, qcol0:qcol0 + K.Q].reshape(B, N, K.Q)
    if dq_rows is not None:
        dS, Qv = dS[:, :dq_rows], Qv[:, :dq_rows]
    return (torch.einsum("bnc,bnk->bck", dS, Qv) * sc).reshape(B * C, K.Q)


def gather_rows(src, m, B, C, N, col0, width):
    return src.view(B, N, -1)[torch.arange(B)[:, None], m.long(), col0:col0 + width].reshape(B * C, width).contiguous()


def dsmil_qv(X, m, wq, bq, B, N, C):
    if X.shape[-1] > 2048:
        raise RuntimeError("dsmil_qv")
    xm = X[torch.arange(B)[:, None], m.long()].reshape(B * C, -1).float()
    q = xm @ wq.t() + bq
    return xm, q, q @ wq


def dsmil_qv_bwd(R, qmax, xm, wq, dcmax=None, dwc=None, dbc=None, accumulate=True, *, ignore_accumulate=False):
    dq = R @ wq.t()
    dwq, dbq = qmax.t() @ R + dq.t() @ xm, dq.sum(0)
    if dcmax is not None:
        B, C = dcmax.shape
        w, b = torch.einsum("bc,bcd->cd", dcmax, xm.view(B, C, -1)), dcmax.sum(0)
        if accumulate and not ignore_accumulate:
            dwc += w
            dbc += b
        else:
            dwc.copy_(w)
            dbc.copy_(b)
    return dwq, dbq


def rows_dot_wsum(X, V, G):
    B, N, d = X.shape
    C = V.shape[1]
    if C > 2 or d > 1024 or d % 8 or N % 4:                          # what the plan refuses (rows_per_wave >= 4 divides N)
        return None
    return rows_dot(X, V), torch.einsum("bnc,bnd->cd", G, X.float())


def topk_ids(A, k, *, highest_wins=False):
    if k > 32 or k > A.shape[1]:
        raise RuntimeError("topk_ids")
    N = A.shape[1]
    a = A.flip(1) if highest_wins else A
    top = torch.sort(a, dim=1, descending=True, stable=True)[1][:, :k]
    bot = torch.sort(a, dim=1, descending=False, stable=True)[1][:, :k]
    ids = torch.cat([top, bot], 1)
    return (N - 1 - ids if highest_wins else ids).to(torch.int32)


def clam_inst_fwd(h, ids, labels, W, bias, B, N, k, n_cls, subtyping):
    R, scale = 2 * k, (1.0 / n_cls if subtyping else 1.0)
    rows = (torch.arange(B)[:, None] * N + ids.long()).reshape(-1)
    x = (h[rows].float() @ W.t() + bias).view(B, R, n_cls, 2).permute(0, 2, 1, 3)                     # [B, n_cls, R, 2]
    own = (torch.arange(n_cls)[None, :] == labels[:, None])[:, :, None]                                # [B, n_cls, 1]
    top = (torch.arange(R) < k)[None, None, :]
    t = torch.where(own, top.long(), torch.where(top & bool(subtyping), 0, -1)).expand(B, n_cls, R)
    live = t >= 0
    cnt = live.sum(2, keepdim=True).clamp_min(1).float()
    lsm = torch.log_softmax(x, 3)
    onehot = torch.nn.functional.one_hot(t.clamp_min(0), 2).float()
    ce = -(lsm * onehot).sum(3) * live / cnt
    dl = (lsm.exp() - onehot) * (live / cnt)[..., None] * scale
    pred = torch.where(live, (x[..., 1] > x[..., 0]).long(), -1)
    return ce.sum((1, 2)) * scale, dl.permute(0, 2, 1, 3).reshape(B * R, 2 * n_cls), torch.stack([pred, t])


def take_rows(src, rows):
    return src[rows].float()


def scatter_add_rows_masked(dst, h, rows, g, write_back=False):
    on = h[rows].float() > 0
    add = torch.where(on, g, torch.zeros(()))
    dst[rows] = (dst[rows].float() + add).to(dst.dtype)
    if write_back:
        g.copy_(add)


def cross_entropy(logits, targets, group, want_conf=False, *, by_group_size=False):
    R, C = logits.shape
    live = targets >= 0
    cnt = live.view(-1, group).sum(1).float()
    inv = torch.where(cnt > 0, 1.0 / (torch.full_like(cnt, group) if by_group_size else cnt.clamp_min(1)), torch.zeros(()))
    lsm = torch.log_softmax(logits, 1)
    tc = targets.clamp_min(0)
    row = torch.where(live, -lsm.gather(1, tc[:, None])[:, 0], torch.zeros(()))
    loss = row.view(-1, group).sum(1) * inv
    dl = (lsm.exp() - torch.nn.functional.one_hot(tc, C).float()) * (live * inv.repeat_interleave(group))[:, None]
    first = (logits == logits.max(1, keepdim=True)[0]).float().argmax(1)                               # the first maximum
    preds = torch.where(live, first, -1)
    conf = torch.where(live, lsm.gather(1, tc[:, None])[:, 0].exp(), torch.zeros(()))
    return (loss, dl, preds, conf) if want_conf else (loss, dl, preds)


def group_mean(x, groups, group):
    return x.view(groups, group).mean(1)


def mul(x, k, out=None):
    out = x if out is None else out
    return out.copy_(x * k)


EMU = dict(rows_dot=rows_dot, weighted_rowsum=weighted_rowsum, dsmil_softmax_=dsmil_softmax_, dsmil_softmax_bwd=dsmil_softmax_bwd,
           dsmil_attn=dsmil_attn, dsmil_attn_bwd=dsmil_attn_bwd, gather_rows=gather_rows, dsmil_qv=dsmil_qv, dsmil_qv_bwd=dsmil_qv_bwd,
           rows_dot_wsum=rows_dot_wsum, topk_ids=topk_ids, clam_inst_fwd=clam_inst_fwd, take_rows=take_rows,
           scatter_add_rows_masked=scatter_add_rows_masked, cross_entropy=cross_entropy, group_mean=group_mean, mul=mul)


def _with(fn, **defect):
    return lambda *a, **kw: fn(*a, **kw, **defect)


# ------------------------------------------------------------------ the emulation passes every check
@pytest.mark.parametrize("family", list(K.FAMILIES))
def test_the_f32_emulation_passes_every_check(family):
    check, entry, cases = K.FAMILIES[family]
    extra = dict(rows_dot=rows_dot) if family == "rows_dot_wsum" else {}
    for args in cases:
        check(EMU[entry], CPU, *args, **extra)
    if family == "dsmil_attn_bwd":
        assert [c for c in K.ATTN_BWD_CASES if c[2] > 4 and c[3] > K.Q], "a class-group case with columns outside the slice"


def test_the_emulation_refuses_what_the_entry_points_refuse():
    with pytest.raises(RuntimeError):
        dsmil_softmax_(torch.zeros(2, 8, 5))
    for N, k in ((64, 33), (8, 9)):
        with pytest.raises(RuntimeError):
            topk_ids(torch.zeros(2, N), k)
    with pytest.raises(RuntimeError):
        dsmil_qv(torch.zeros(1, 4, 2052), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(K.Q, 2052), torch.zeros(K.Q), 1, 4, 2)


# ------------------------------------------------------------------ every defect fails its check
def _unrounded_rows_dot(case):
    raw = K.rows_dot_inputs(case, F32)[0]                           # the values before their rounding to bf16
    return lambda X, V, bias=None: rows_dot(raw, V, bias)


RD, WR, AT = K.ROWS_DOT_CASES[1], K.WEIGHTED_ROWSUM_CASES[1], K.ATTN_CASES[1]
DEFECTS = {
    "rows_dot drops the last row of each bag": lambda: K.check_rows_dot(_with(rows_dot, drop_last=True), CPU, RD, F32, False),
    "weighted_rowsum drops the last row of each bag": lambda: K.check_weighted_rowsum(_with(weighted_rowsum, drop_last=True), CPU, WR, BF16),
    "dsmil_attn ignores qcol0": lambda: K.check_dsmil_attn(_with(dsmil_attn, use_qcol0=False), CPU, AT),
    "dsmil_attn scales by 1/128": lambda: K.check_dsmil_attn(_with(dsmil_attn, scale=1.0 / K.Q), CPU, K.ATTN_CASES[0]),
    "topk_ids: highest index wins ties": lambda: K.check_topk_ids(_with(topk_ids, highest_wins=True), CPU, (2, 4097, 8), "ties"),
    "dsmil_qv_bwd_cls ignores accumulate": lambda: K.check_dsmil_qv_bwd_cls(_with(dsmil_qv_bwd, ignore_accumulate=True), CPU, K.QV_CASES[1]),
    "weighted_rowsum into= clears": lambda: K.check_weighted_rowsum_into(_with(weighted_rowsum, clears=True), CPU, WR, F32),
    "cross_entropy divides by the group size": lambda: K.check_cross_entropy(_with(cross_entropy, by_group_size=True), CPU, K.CE_CASES[3]),
    "dqmax misses the rows past the first 64 (N = 70)": lambda: K.check_dsmil_attn_bwd(_with(dsmil_attn_bwd, dq_rows=64), CPU, AT),
    "dqmax misses the rows past the first 64 (N = 130, class groups)": lambda: K.check_dsmil_attn_bwd(_with(dsmil_attn_bwd, dq_rows=64), CPU, K.ATTN_CASES[2]),
    "bf16 input read as if unrounded": lambda: K.check_rows_dot(_unrounded_rows_dot(RD), CPU, RD, BF16, False),
    "dsmil_attn_bwd touches dY outside its slice": lambda: K.check_dsmil_attn_bwd(_with(dsmil_attn_bwd, whole_rows=True), CPU, K.ATTN_CASES[2]),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_a_defective_emulation_fails_its_check(defect):
    with pytest.raises(AssertionError):
        DEFECTS[defect]()
