"""The C-ABI calls of the DSMIL aggregator (``DSMILFn``: one forward chain, one staged backward, the route chosen once by
``functional.dsmil_route``), per route and mode, by name.

The recorder is that of tests/test_gpu_gru_launches.py: it wraps ``ops.check``, through which every C-ABI call of ops.py passes with
its name.  The sequences below were recorded with it, on an MI355X, from commit 3ceb533, whose ``DSMILFn`` chose its path twice (forward
and backward each asked the kernels' plan and four module switches) and threaded flags through a five-arm backward; they pin what
the staged node must call: exactly, in order.  The routes are reached through shapes, so the lists are what real inputs launch:

  stream     B = 2, N = 64, d = 64, C = 2 (f32 and bf16): the one-pass kernels cover it;
  explicit   C = 3 (the stream plan takes C <= 2) and N = 66 (it takes N % 4 == 0), both with ``dsmil_qv`` in front; d = 2056 (past
             ``dsmil_qv``'s 2048) without it; and the stream shape with a keep mask on the value branch ("dropped");
  literal    C = 5.  3ceb533 has no list for it: its row kernels refuse C > 4 ("rows_dot failed with code -1" in the first launch),
             and ops.py now launches them per group of four classes, so these two lists are this commit's own - the names of
             "literal.forced.c2" with the row kernels doubled - and pin it for later changes; they say nothing about 3ceb533.  "literal.forced.c2" runs the route where the parity test of
             tests/test_gpu_modules.py does: at C = 2, with ``dsmil_route`` overridden - recorded at 3ceb533 with its module switch for
             the reassociated order off.

Each case runs the forward and the backward of ``(bag * wb).sum() + (classes * wc).sum()`` unless its name says otherwise ("cmax": the
max-instance scores of ``want_max=True`` alone, with the dense ``classes`` term, with the bag term; "classes_only": no bag gradient),
"plain" (autograd accumulates) or "direct" (a ``FlatAdam`` seats the gradients and the kernels add into them), or the forward alone
under ``torch.no_grad()``.  (A name says which entry ran, not on what: tests/test_gpu_modules.py holds the numbers.)
"""
import pytest
import torch

from oracle import detrand, params as P

pytestmark = pytest.mark.gpu

SEED = 37
STREAM, C3, N66, D2056, C5 = (2, 64, 64, 2), (2, 64, 64, 3), (2, 66, 64, 2), (2, 64, 2056, 2), (2, 64, 64, 5)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def hooks(monkeypatch):
    """Every module-level switch of functional.py that the node reads at its default, whatever an earlier test left behind."""
    from murcl_amd import functional
    for name, value in [("_DIRECT", False), ("_MILESTONE", None), ("_DEFER_ON", True), ("_DEFERRED", None)]:
        monkeypatch.setattr(functional, name, value)
    return monkeypatch


def _calls(hooks, body):
    """The ``what`` of every ``ops.check`` while ``body`` runs."""
    from murcl_amd import ops
    names, real = [], ops.check

    def check(rc, what):
        names.append(what)
        return real(rc, what)
    hooks.setattr(ops, "check", check)
    body()
    torch.cuda.synchronize()
    hooks.setattr(ops, "check", real)
    return names


def _rand(tag, shape):
    return torch.from_numpy(detrand.normal(SEED, f"dl.{tag}", shape)).to(_dev())


def _run(hooks, shape, dtype=torch.float32, mode="plain", loss="bag+classes", dropped=False, force=None):
    from murcl_amd import functional
    from murcl_amd.models.dsmil import build_dsmil
    from murcl_amd.optim import FlatAdam
    B, N, d, C = shape
    m = build_dsmil(d, C)
    m.load_state_dict(P.to_torch(P.dsmil(SEED, d, C)))
    m.compute_dtype = dtype
    m = m.to(_dev())
    x = torch.from_numpy(P.bags(SEED, f"dl.x{N}.{d}", B, N, d)).to(_dev()).to(dtype)
    if dropped:
        m.keep_mask_v = ((torch.from_numpy(detrand.uniform(SEED, "dl.keep", (B, N, d))) >= 0.25).float() / 0.75).to(_dev())
    if force is not None:
        hooks.setattr(functional, "dsmil_route", lambda *a: functional.DSMILRoute(*force))
    if mode == "direct":
        opt = FlatAdam([{"params": list(m.parameters()), "lr": 1e-4}])       # noqa: F841  (owns the gradient buffer)
        assert functional._DIRECT and all(p.grad is not None for p in m.parameters())
    terms = {"bag": lambda o: (o[1] * _rand("wb", (B, C, d))).sum(), "classes": lambda o: (o[0] * _rand("wc", (B, N, C))).sum(),
             "cmax": lambda o: (o[2] * _rand("wm", (B, C))).sum()}

    def body():
        if mode == "no_grad":
            with torch.no_grad():
                out = m._run(x)
            assert not out[1].requires_grad
        else:
            out = m._run(x, want_max="cmax" in loss)
            sum(terms[t](out) for t in loss.split("+")).backward()
    return _calls(hooks, body)


CASES = {
    "stream.f32.plain": dict(shape=STREAM),
    "stream.f32.direct": dict(shape=STREAM, mode="direct"),
    "stream.bf16.plain": dict(shape=STREAM, dtype=torch.bfloat16),
    "stream.bf16.direct": dict(shape=STREAM, dtype=torch.bfloat16, mode="direct"),
    "stream.cmax.plain": dict(shape=STREAM, loss="cmax"),
    "stream.cmax+classes.plain": dict(shape=STREAM, loss="cmax+classes"),
    "stream.bag+cmax.plain": dict(shape=STREAM, loss="bag+cmax"),
    "stream.bag+cmax.direct": dict(shape=STREAM, loss="bag+cmax", mode="direct"),
    "stream.classes_only.plain": dict(shape=STREAM, loss="classes"),
    "stream.no_grad": dict(shape=STREAM, mode="no_grad"),
    "dropped.f32.plain": dict(shape=STREAM, dropped=True),
    "explicit.c3.plain": dict(shape=C3),
    "explicit.c3.direct": dict(shape=C3, mode="direct"),
    "explicit.c3.cmax.plain": dict(shape=C3, loss="cmax"),
    "explicit.c3.cmax+classes.plain": dict(shape=C3, loss="cmax+classes"),
    "explicit.c3.classes_only.plain": dict(shape=C3, loss="classes"),
    "explicit.c3.no_grad": dict(shape=C3, mode="no_grad"),
    "explicit.n66.plain": dict(shape=N66),
    "explicit.d2056.noqv.plain": dict(shape=D2056),
    "literal.c5.plain": dict(shape=C5),
    "literal.c5.no_grad": dict(shape=C5, mode="no_grad"),
    "literal.forced.c2.plain": dict(shape=STREAM, force=(False, False, False)),
    "literal.forced.c2.bf16.plain": dict(shape=STREAM, dtype=torch.bfloat16, force=(False, False, False)),
}

RECORDED = {
    "stream.f32.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "dsmil_attn_pool_bwd", "colsum", "dsmil_qv_bwd"
    ],
    "stream.f32.direct": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt", "gemm_tn_grouped", "cast_batch", "gemm_nt",
        "dsmil_attn_pool_bwd", "colsum", "dsmil_qv_bwd", "add_lists"
    ],
    "stream.bf16.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "dsmil_attn_pool_bwd", "colsum", "dsmil_qv_bwd"
    ],
    "stream.bf16.direct": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt", "gemm_tn_grouped", "cast_batch", "gemm_nt",
        "dsmil_attn_pool_bwd", "colsum", "dsmil_qv_bwd", "add_lists"
    ],
    "stream.cmax.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "dsmil_attn_pool_bwd", "dsmil_qv_bwd_cls"
    ],
    "stream.cmax+classes.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "dsmil_attn_pool_bwd", "colsum", "dsmil_qv_bwd_cls"
    ],
    "stream.bag+cmax.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "dsmil_attn_pool_bwd", "dsmil_qv_bwd_cls"
    ],
    "stream.bag+cmax.direct": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt", "gemm_tn_grouped", "cast_batch", "gemm_nt",
        "dsmil_attn_pool_bwd", "dsmil_qv_bwd_cls", "add_lists"
    ],
    "stream.classes_only.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "dsmil_attn_pool_bwd", "colsum", "dsmil_qv_bwd"
    ],
    "stream.no_grad": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "dsmil_attn_pool", "gemm_nt"
    ],
    "dropped.f32.plain": [
        "mul", "rows_dot", "dsmil_argmax_max", "dsmil_qv", "rows_dot", "dsmil_softmax", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "transpose_cast", "gemm_nt", "rows_dot", "dsmil_softmax_bwd", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "gemm_tn_grouped", "colsum", "weighted_rowsum"
    ],
    "explicit.c3.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "rows_dot", "dsmil_softmax", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "transpose_cast", "gemm_nt", "rows_dot", "dsmil_softmax_bwd", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "gemm_tn_grouped", "colsum", "weighted_rowsum"
    ],
    "explicit.c3.direct": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "rows_dot", "dsmil_softmax", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "cast_batch", "gemm_nt", "rows_dot", "dsmil_softmax_bwd", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped", "gemm_tn_grouped",
        "colsum", "weighted_rowsum", "add_lists"
    ],
    "explicit.c3.cmax.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "rows_dot", "dsmil_softmax", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "transpose_cast", "gemm_nt", "rows_dot", "dsmil_softmax_bwd", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "gemm_tn_grouped", "colsum"
    ],
    "explicit.c3.cmax+classes.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "rows_dot", "dsmil_softmax", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "transpose_cast", "gemm_nt", "rows_dot", "dsmil_softmax_bwd", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "gemm_tn_grouped", "colsum", "weighted_rowsum"
    ],
    "explicit.c3.classes_only.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "rows_dot", "dsmil_softmax", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "transpose_cast", "gemm_nt", "rows_dot", "dsmil_softmax_bwd", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "gemm_tn_grouped", "colsum", "weighted_rowsum"
    ],
    "explicit.c3.no_grad": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "rows_dot", "dsmil_softmax", "weighted_rowsum", "gemm_nt"
    ],
    "explicit.n66.plain": [
        "rows_dot", "dsmil_argmax_max", "dsmil_qv", "rows_dot", "dsmil_softmax", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "transpose_cast", "gemm_nt", "rows_dot", "dsmil_softmax_bwd", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "gemm_tn_grouped", "colsum", "weighted_rowsum"
    ],
    "explicit.d2056.noqv.plain": [
        "rows_dot", "dsmil_argmax_max", "gather_rows", "pad_cols", "pad_cols", "gemm_nt", "transpose_cast", "gemm_nt", "rows_dot",
        "dsmil_softmax", "weighted_rowsum", "pad_cols", "pad_cols", "gemm_nt", "gemm_tn_grouped", "transpose_cast", "pad_cols",
        "pad_cols", "gemm_nt", "gather_rows", "rows_dot", "dsmil_softmax_bwd", "weighted_rowsum", "pad_cols", "pad_cols", "gemm_nt",
        "gemm_tn_grouped", "gemm_tn_grouped", "colsum", "weighted_rowsum"
    ],
    "literal.c5.plain": [
        "rows_dot", "rows_dot", "dsmil_argmax_max", "gemm_nt", "gather_rows", "dsmil_attn", "dsmil_attn", "weighted_rowsum",
        "weighted_rowsum", "gemm_nt", "gemm_tn_grouped", "transpose_cast", "gemm_nt", "gather_rows", "rows_dot", "rows_dot",
        "dsmil_attn_bwd", "dsmil_attn_bwd", "gemm_tn_grouped", "colsum", "gemm_tn_grouped", "colsum", "weighted_rowsum",
        "weighted_rowsum"
    ],
    "literal.c5.no_grad": [
        "rows_dot", "rows_dot", "dsmil_argmax_max", "gemm_nt", "gather_rows", "dsmil_attn", "dsmil_attn", "weighted_rowsum",
        "weighted_rowsum", "gemm_nt"
    ],
    "literal.forced.c2.plain": [
        "rows_dot", "dsmil_argmax_max", "gemm_nt", "gather_rows", "dsmil_attn", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "transpose_cast", "gemm_nt", "gather_rows", "rows_dot_wsum", "colsum", "dsmil_attn_bwd", "gemm_tn_grouped", "colsum",
        "gemm_tn_grouped", "colsum"
    ],
    "literal.forced.c2.bf16.plain": [
        "rows_dot", "dsmil_argmax_max", "cast", "gemm_nt", "gather_rows", "dsmil_attn", "weighted_rowsum", "gemm_nt", "gemm_tn_grouped",
        "transpose_cast", "gemm_nt", "gather_rows", "rows_dot_wsum", "colsum", "dsmil_attn_bwd", "cast", "gemm_tn_grouped", "colsum",
        "cast", "gemm_tn_grouped", "colsum"
    ],
}


@pytest.mark.parametrize("name", list(CASES))
def test_call_sequence_is_the_recorded_one(name, hooks):
    assert _run(hooks, **CASES[name]) == RECORDED[name]


def test_route_by_shape():
    """The shapes above take the routes their names say (and the bench shape the stream route)."""
    from murcl_amd.functional import dsmil_route
    assert dsmil_route(*STREAM, False) == (True, True, True) and dsmil_route(16, 8192, 1024, 2, False) == (True, True, True)
    assert dsmil_route(*STREAM, True) == dsmil_route(*C3, False) == dsmil_route(*N66, False) == (True, True, False)
    assert dsmil_route(*D2056, False) == (True, False, False) and dsmil_route(*C5, False) == (False, False, False)
