"""The C-ABI calls of the recurrent head (``Full_layer``: one GRU forward chain, one backward), per entry point and mode, by name.

The GRU ops open no ``ops.TIMERS`` span, so the recorder wraps ``ops.check``: every C-ABI call of ops.py passes through it with its
name.  The sequences below were recorded with this recorder from commit 80f98ec, which spelled the head out per layout
(``GRUStepFn``, ``GRUSeqFn``, ``GRUViewSeqFn`` and three forward-only copies in models/rlmil.py); they pin what the shared chain must
call: exactly, in order.  (Recorded on a host without a device, the return codes ignored: which entry is called when is host logic -
shapes, modes, ``ops.gru_step_ok``, the weight-gradient plan query - and reads nothing off the device.)  Each case runs the forward and the backward of ``(out * w).sum()`` ("plain": autograd accumulates;
"direct": a ``FlatAdam`` seats the gradients and the kernels add into them), or the forward alone under ``torch.no_grad()``.
The "unfused" cases force ``ops.gru_step_ok`` to False: ``gemm_nt`` + gate kernel per step, which otherwise only an H that is no
multiple of 16 reaches.  (A name says which entry ran, not on what: tests/test_gpu_kernels.py and
tests/test_gpu_autograd_contract.py hold the numbers.)

Shapes: B = 8 rows (a ragged 16-row tile), I = H = 32, T = 3; 6, 3 and 2 blocks for the view sequence (the node's minimum is 3).
"""
import contextlib

import pytest
import torch

from oracle import detrand, params as P

pytestmark = pytest.mark.gpu

SEED = 31
B, I, H, C, T = 8, 32, 32, 16, 3
ONE_LAUNCH = ("gru_step_fwd", "gru_step_bwd")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def hooks(monkeypatch):
    """Every module-level switch of functional.py that the head reads at its default, whatever an earlier test left behind."""
    from murcl_amd import functional
    for name, value in [("_DIRECT", False), ("_MILESTONE", None), ("_DEFER_ON", True), ("_DEFERRED", None)]:
        monkeypatch.setattr(functional, name, value)
    return monkeypatch


def _head():
    from murcl_amd.models.rlmil import Full_layer
    fc = Full_layer(I, H, True, C)
    fc.load_state_dict(P.to_torch(P.full_layer(SEED, I, H, C)))
    return fc.to(_dev())


def _x(tag, rows=B, grad=True):
    return torch.from_numpy(detrand.normal(SEED, f"gl.{tag}", (rows, I))).to(_dev()).requires_grad_(grad)


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


# ---------------------------------------------------------------- the entry points: (fc, grad) -> z
def fwd_restart(fc, grad):
    return fc(_x("a", grad=grad), restart=True)


def fwd_pair(fc, grad):
    return torch.cat([fc(_x("b0", grad=grad), restart=True), fc(_x("b1", grad=grad))], 0)


def fwd_seq(fc, grad, steps=T):
    return fc.forward_sequence(_x("c", steps * B, grad).view(steps, B, I))


def fwd_seq1(fc, grad):
    return fwd_seq(fc, grad, 1)


def _view_seq(n, whole):
    def fwd(fc, grad):
        if not whole:                                             # separately allocated aggregator outputs
            return fc.forward_view_sequence([_x(f"e{k}", grad=grad) for k in range(n)])
        h = _x("e", n * B, grad)
        h = h * 1.0 if grad else h                                # row blocks of one (non-leaf) tensor, as CL.forward hands them out
        return fc.forward_view_sequence(list(h.split(B, 0)), whole=h)
    return fwd


def fwd_views(fc, grad):
    return torch.cat(fc.forward_views([_x("g0", grad=grad), _x("g1", grad=grad)], restart=True), 0)


def _run(hooks, fwd, mode, deferred=False, unfused=False):
    from murcl_amd import functional, ops
    from murcl_amd.optim import FlatAdam
    fc = _head()
    w = torch.from_numpy(detrand.normal(SEED, "gl.w", (6 * B, C))).to(_dev())
    if unfused:
        hooks.setattr(ops, "gru_step_ok", lambda *a, **k: False)
    if mode == "direct":
        opt = FlatAdam([{"params": list(fc.parameters()), "lr": 1e-4}])      # noqa: F841  (owns the gradient buffer)
        assert functional._DIRECT and all(p.grad is not None for p in fc.parameters())

    def body():
        if mode == "no_grad":
            with torch.no_grad():
                assert not fwd(fc, False).requires_grad
            return
        with functional.deferred_wgrads() if deferred else contextlib.nullcontext():
            z = fwd(fc, True)
            (z * w[:z.shape[0]]).sum().backward()
    return _calls(hooks, body)


CASES = {
    "a.restart.plain": (fwd_restart, dict(mode="plain")),
    "a.restart.direct": (fwd_restart, dict(mode="direct")),
    "b.pair.plain": (fwd_pair, dict(mode="plain")),
    "b.pair.direct_deferred": (fwd_pair, dict(mode="direct", deferred=True)),
    "c.seq.plain": (fwd_seq, dict(mode="plain")),
    "c.seq.direct": (fwd_seq, dict(mode="direct")),
    "d.seq_T1.direct": (fwd_seq1, dict(mode="direct")),
    "e.views6.whole.plain": (_view_seq(6, True), dict(mode="plain")),
    "e.views6.whole.direct": (_view_seq(6, True), dict(mode="direct")),
    "e.views6.plain": (_view_seq(6, False), dict(mode="plain")),
    "e.views6.direct": (_view_seq(6, False), dict(mode="direct")),
    "e.views3.whole.plain": (_view_seq(3, True), dict(mode="plain")),
    "e.views3.whole.direct": (_view_seq(3, True), dict(mode="direct")),
    "e.views3.plain": (_view_seq(3, False), dict(mode="plain")),
    "e.views3.direct": (_view_seq(3, False), dict(mode="direct")),
    "f.views2.plain": (_view_seq(2, False), dict(mode="plain")),
    "f.views2.direct": (_view_seq(2, False), dict(mode="direct")),
    "g.forward_views.plain": (fwd_views, dict(mode="plain")),
    "g.forward_views.direct": (fwd_views, dict(mode="direct")),
    "h.restart.no_grad": (fwd_restart, dict(mode="no_grad")),
    "h.pair.no_grad": (fwd_pair, dict(mode="no_grad")),
    "h.seq.no_grad": (fwd_seq, dict(mode="no_grad")),
    "h.views6.whole.no_grad": (_view_seq(6, True), dict(mode="no_grad")),
    "h.views6.no_grad": (_view_seq(6, False), dict(mode="no_grad")),
    "h.views3.whole.no_grad": (_view_seq(3, True), dict(mode="no_grad")),
    "h.views3.no_grad": (_view_seq(3, False), dict(mode="no_grad")),
    "h.forward_views.no_grad": (fwd_views, dict(mode="no_grad")),
    "i.pair.unfused.plain": (fwd_pair, dict(mode="plain", unfused=True)),
    "i.pair.unfused.direct_deferred": (fwd_pair, dict(mode="direct", deferred=True, unfused=True)),
    "i.seq.unfused.plain": (fwd_seq, dict(mode="plain", unfused=True)),
    "i.seq.unfused.direct": (fwd_seq, dict(mode="direct", unfused=True)),
}

RECORDED = {
    "a.restart.plain": [
        "gru_step_fwd", "gemm_nt", "transpose_cast", "gemm_nt_smallk", "gemm_tn_grouped", "colsum", "gru_gates_bwd",
        "transpose_cast", "gemm_nt", "gemm_tn_grouped", "colsum", "colsum"
    ],
    "a.restart.direct": [
        "gru_step_fwd", "gemm_nt", "cast_batch", "gemm_nt_smallk", "gemm_tn_grouped", "gru_gates_bwd", "cast_batch", "gemm_nt",
        "gemm_tn_grouped", "colsum"
    ],
    "b.pair.plain": [
        "gru_step_fwd", "gemm_nt", "gemm_nt", "gru_step_fwd", "gemm_nt", "transpose_cast", "gemm_nt_smallk", "gemm_tn_grouped",
        "colsum", "gru_gates_bwd", "transpose_cast", "gemm_nt", "gemm_tn_grouped", "colsum", "gemm_tn_grouped", "colsum",
        "transpose_cast", "gemm_nt", "transpose_cast", "gemm_nt_smallk", "gemm_tn_grouped", "colsum", "gru_gates_bwd",
        "transpose_cast", "gemm_nt", "gemm_tn_grouped", "colsum", "colsum"
    ],
    "b.pair.direct_deferred": [
        "gru_step_fwd", "gemm_nt", "gemm_nt", "gru_step_fwd", "gemm_nt", "cast_batch", "gemm_nt_smallk", "gru_gates_bwd",
        "cast_batch", "gemm_nt", "cast_batch", "gemm_nt", "gemm_nt_smallk", "gru_gates_bwd", "gemm_nt", "colsum", "gemm_tn_grouped"
    ],
    "c.seq.plain": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gru_step_fwd", "gemm_nt", "transpose_cast", "gemm_nt_smallk",
        "gemm_tn_grouped", "colsum", "transpose_cast", "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd", "gru_step_bwd",
        "transpose_cast", "gemm_nt", "gemm_tn_grouped", "gemm_tn_grouped", "colsum", "colsum"
    ],
    "c.seq.direct": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gru_step_fwd", "gemm_nt", "cast_batch", "gemm_nt_smallk", "gemm_tn_grouped",
        "cast_batch", "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd", "gru_step_bwd", "cast_batch", "gemm_nt",
        "gemm_tn_grouped", "gemm_tn_grouped", "colsum", "colsum"
    ],
    "d.seq_T1.direct": [
        "gemm_nt", "gru_gates_fwd", "gemm_nt", "cast_batch", "gemm_nt_smallk", "gemm_tn_grouped", "cast_batch", "gru_gates_bwd",
        "cast_batch", "gemm_nt", "gemm_tn_grouped", "colsum", "colsum"
    ],
    "e.views6.whole.plain": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gemm_nt", "transpose_cast",
        "gemm_nt_smallk", "gemm_tn_grouped", "colsum", "transpose_cast", "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd",
        "gru_step_bwd", "gru_step_bwd", "gru_step_bwd", "gru_gates_bwd_into", "transpose_cast", "gemm_nt", "gemm_tn_grouped",
        "colsum", "gemm_tn_grouped", "colsum"
    ],
    "e.views6.whole.direct": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gemm_nt", "cast_batch",
        "gemm_nt_smallk", "gemm_tn_grouped", "cast_batch", "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd", "gru_step_bwd",
        "gru_step_bwd", "gru_step_bwd", "gru_gates_bwd_into", "cast_batch", "gemm_nt", "gemm_tn_grouped", "gemm_tn_grouped",
        "colsum"
    ],
    "e.views6.plain": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gemm_nt", "transpose_cast",
        "gemm_nt_smallk", "gemm_tn_grouped", "colsum", "transpose_cast", "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd",
        "gru_step_bwd", "gru_step_bwd", "gru_step_bwd", "gru_gates_bwd_into", "transpose_cast", "gemm_nt", "gemm_tn_grouped",
        "colsum", "gemm_tn_grouped", "colsum"
    ],
    "e.views6.direct": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gemm_nt", "cast_batch",
        "gemm_nt_smallk", "gemm_tn_grouped", "cast_batch", "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd", "gru_step_bwd",
        "gru_step_bwd", "gru_step_bwd", "gru_gates_bwd_into", "cast_batch", "gemm_nt", "gemm_tn_grouped", "gemm_tn_grouped",
        "colsum"
    ],
    "e.views3.whole.plain": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gemm_nt", "transpose_cast", "gemm_nt_smallk", "gemm_tn_grouped", "colsum",
        "transpose_cast", "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd", "gru_gates_bwd_into", "transpose_cast", "gemm_nt",
        "gemm_tn_grouped", "colsum", "gemm_tn_grouped", "colsum"
    ],
    "e.views3.whole.direct": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gemm_nt", "cast_batch", "gemm_nt_smallk", "gemm_tn_grouped", "cast_batch",
        "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd", "gru_gates_bwd_into", "cast_batch", "gemm_nt", "gemm_tn_grouped",
        "gemm_tn_grouped", "colsum"
    ],
    "e.views3.plain": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gemm_nt", "transpose_cast", "gemm_nt_smallk", "gemm_tn_grouped", "colsum",
        "transpose_cast", "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd", "gru_gates_bwd_into", "transpose_cast", "gemm_nt",
        "gemm_tn_grouped", "colsum", "gemm_tn_grouped", "colsum"
    ],
    "e.views3.direct": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gemm_nt", "cast_batch", "gemm_nt_smallk", "gemm_tn_grouped", "cast_batch",
        "copy_bytes", "gru_gates_bwd_into", "gru_step_bwd", "gru_gates_bwd_into", "cast_batch", "gemm_nt", "gemm_tn_grouped",
        "gemm_tn_grouped", "colsum"
    ],
    "f.views2.plain": [
        "gru_step_fwd", "gemm_nt", "gru_gates_fwd", "gemm_nt", "transpose_cast", "gemm_nt_smallk", "gemm_tn_grouped", "colsum",
        "transpose_cast", "gru_gates_bwd", "transpose_cast", "gemm_nt", "gemm_tn_grouped", "colsum", "colsum", "gru_gates_bwd",
        "transpose_cast", "gemm_nt", "gemm_tn_grouped", "colsum", "colsum"
    ],
    "f.views2.direct": [
        "gru_step_fwd", "gemm_nt", "gru_gates_fwd", "gemm_nt", "cast_batch", "gemm_nt_smallk", "gemm_tn_grouped", "cast_batch",
        "gru_gates_bwd", "cast_batch", "gemm_nt", "gemm_tn_grouped", "colsum", "colsum", "gru_gates_bwd", "gemm_nt",
        "gemm_tn_grouped", "colsum"
    ],
    "g.forward_views.plain": [
        "gru_step_fwd", "gemm_nt", "transpose_cast", "gemm_nt_smallk", "gemm_tn_grouped", "colsum", "gru_gates_bwd",
        "transpose_cast", "gemm_nt", "gemm_tn_grouped", "colsum", "colsum"
    ],
    "g.forward_views.direct": [
        "gru_step_fwd", "gemm_nt", "cast_batch", "gemm_nt_smallk", "gemm_tn_grouped", "gru_gates_bwd", "cast_batch", "gemm_nt",
        "gemm_tn_grouped", "colsum"
    ],
    "h.restart.no_grad": [
        "gru_step_fwd", "gemm_nt"
    ],
    "h.pair.no_grad": [
        "gru_step_fwd", "gemm_nt", "gru_step_fwd", "gemm_nt"
    ],
    "h.seq.no_grad": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gru_step_fwd", "gemm_nt"
    ],
    "h.views6.whole.no_grad": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gemm_nt"
    ],
    "h.views6.no_grad": [
        "stack_lists", "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gru_step_fwd", "gemm_nt"
    ],
    "h.views3.whole.no_grad": [
        "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gemm_nt"
    ],
    "h.views3.no_grad": [
        "stack_lists", "gemm_nt", "gru_gates_fwd", "gru_step_fwd", "gemm_nt"
    ],
    "h.forward_views.no_grad": [
        "gru_step_fwd", "gemm_nt"
    ],
    "i.pair.unfused.plain": [
        "gemm_nt", "gru_gates_fwd", "gemm_nt", "gemm_nt", "gemm_nt", "gru_gates_fwd", "gemm_nt", "transpose_cast", "gemm_nt_smallk",
        "gemm_tn_grouped", "colsum", "gru_gates_bwd", "transpose_cast", "gemm_nt", "gemm_tn_grouped", "colsum", "gemm_tn_grouped",
        "colsum", "transpose_cast", "gemm_nt", "transpose_cast", "gemm_nt_smallk", "gemm_tn_grouped", "colsum", "gru_gates_bwd",
        "transpose_cast", "gemm_nt", "gemm_tn_grouped", "colsum", "colsum"
    ],
    "i.pair.unfused.direct_deferred": [
        "gemm_nt", "gru_gates_fwd", "gemm_nt", "gemm_nt", "gemm_nt", "gru_gates_fwd", "gemm_nt", "cast_batch", "gemm_nt_smallk",
        "gru_gates_bwd", "cast_batch", "gemm_nt", "cast_batch", "gemm_nt", "gemm_nt_smallk", "gru_gates_bwd", "gemm_nt", "colsum",
        "gemm_tn_grouped"
    ],
    "i.seq.unfused.plain": [
        "gemm_nt", "gru_gates_fwd", "gemm_nt", "gru_gates_fwd", "gemm_nt", "gru_gates_fwd", "gemm_nt", "transpose_cast",
        "gemm_nt_smallk", "gemm_tn_grouped", "colsum", "transpose_cast", "gru_gates_bwd", "gemm_nt", "gru_gates_bwd", "gemm_nt",
        "gru_gates_bwd", "transpose_cast", "gemm_nt", "gemm_tn_grouped", "gemm_tn_grouped", "colsum", "colsum"
    ],
    "i.seq.unfused.direct": [
        "gemm_nt", "gru_gates_fwd", "gemm_nt", "gru_gates_fwd", "gemm_nt", "gru_gates_fwd", "gemm_nt", "cast_batch",
        "gemm_nt_smallk", "gemm_tn_grouped", "cast_batch", "gru_gates_bwd", "gemm_nt", "gru_gates_bwd", "gemm_nt", "gru_gates_bwd",
        "cast_batch", "gemm_nt", "gemm_tn_grouped", "gemm_tn_grouped", "colsum", "colsum"
    ],
}


@pytest.mark.parametrize("name", list(CASES))
def test_call_sequence_is_the_recorded_one(name, hooks):
    fwd, how = CASES[name]
    got = _run(hooks, fwd, **how)
    assert got == RECORDED[name]
    if how.get("unfused"):
        assert not set(got) & set(ONE_LAUNCH)
