"""The C-ABI calls of the CLAM aggregator (``CLAMFn``: the route chosen once by ``functional.clam_route``, a staged forward and a staged
backward), per route and mode, by name.

The recorder is that of tests/test_gpu_dsmil_launches.py: it wraps ``ops.check``, through which every C-ABI call of ops.py passes with
its name.  The sequences below were recorded with it, on an MI355X, from commit 0e4675e, whose ``CLAMFn`` decided its path inline - in a
dozen places of one 150-line forward, and again in its backward; they pin what the staged node must call: exactly, in order.

``CLAM_SB(size_arg="small", dropout=True, k_sample=8, n_classes=2)`` (L = 512, D = 256, so 2D = 512) on B = 2 bags of N = 64 patches
of width d = 512 unless the name says otherwise - the smallest shape with B*N % 32 == 0, N % 32 == 0 and ``ops.gated_bwd_il_supported``:

  fused_gate   bf16, eval, ``torch.no_grad()``: the score from the gate GEMM's epilogue; with and without instance evaluation;
  gate_u       bf16 with a backward to follow: eval (the ReLU bit mask from the first layer's epilogue), train with seeded ``DropSeed``s
               (all three Dropouts in the GEMM epilogues), "noinst" (no instance evaluation), "subtyping_off"; "d256": the tile kernel
               as first layer (its Dropout in the bit-mask pass) in front of the same gate;
  separate     bf16 train with ``_GATE_U``, ``_FUSED_FC_DROP`` and ``_FUSED_INST`` off: the chain of separate passes, the
               ``dropout_relu_bitmask`` form, the explicit instance branch;
  injected     bf16 with keep tensors: ``ops.mul`` and ``gated_score_fwd`` with masks;
  f32          eval, and train with seeded drops at N = 66 (no multiple of 32: the Dropout as a materialised mask);
  plain_attn   ``gate=False`` (``Attn_Net``, six gradients) in train mode, f32 and bf16;
  custom_loss  ``instance_loss_fn=nn.CrossEntropyLoss(label_smoothing=0.1)``: the explicit instance branch and its host loop;
  big          B = 2, N = 8192.  ``ops.gemm_tn_grouped_ok`` refuses the two [B*N,512]^T [B*N,512] weight gradients of the gate_u
               backward below B*N = 16384 rows (``murcl_gemm_tn_plan``, asked on the host by ``test_grouped_plan_by_rows``: it picks the
               square-tile kind from there on), so the grouped launch with its deferred column sums is pinned at that shape, with
               ``_GROUP_WGRAD`` on and off, and once with the explicit instance branch behind it.

Each case runs the forward under ``torch.no_grad()`` alone, or the forward and the backward of ``(M * w).sum() + inst_loss.sum()``,
"plain" (autograd accumulates) or "direct" (a ``FlatAdam`` seats the gradients and the kernels add into them).  (A name says which
entry ran, not on what: tests/test_gpu_modules.py holds the numbers.)
"""
import functools

import pytest
import torch

from oracle import detrand, params as P

pytestmark = pytest.mark.gpu

SEED = 41
SMALL, N66, D256, BIG = (2, 64, 512), (2, 66, 512), (2, 64, 256), (2, 8192, 512)
SEPARATE = ("_GATE_U", "_FUSED_FC_DROP", "_FUSED_INST")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def hooks(monkeypatch):
    """Every module-level switch of functional.py that the node reads at its default, whatever an earlier test left behind."""
    from murcl_amd import functional
    for name, value in [("_DIRECT", False), ("_MILESTONE", None), ("_DEFER_ON", True), ("_DEFERRED", None), ("_GROUP_WGRAD", True)]:
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


@functools.lru_cache(maxsize=None)
def _bags(B, N, d):
    """The bags of a shape, generated once for all its cases (read only)."""
    return torch.from_numpy(P.bags(SEED, f"cl.x{N}.{d}", B, N, d)).to(_dev())


def _run(hooks, shape=SMALL, dtype=torch.bfloat16, mode="plain", train=False, keeps=None, inst=True, gate=True, subtyping=True,
         loss_fn=None, off=(), result=None):
    """The calls of one case; ``result`` (a dict) receives its outputs and gradients."""
    from murcl_amd import functional, ops
    from murcl_amd.models.clam import CLAM_SB
    from murcl_amd.optim import FlatAdam
    B, N, d = shape
    m = CLAM_SB(gate=gate, size_arg="small", dropout=True, k_sample=8, n_classes=2, instance_loss_fn=loss_fn, subtyping=subtyping, in_dim=d)
    m.load_state_dict(P.to_torch((P.clam_sb if gate else P.clam_sb_plain)(SEED, in_dim=d)))
    m.compute_dtype = dtype
    m = m.to(_dev()).train(train)
    x = _bags(B, N, d).to(dtype)
    w = torch.from_numpy(detrand.normal(SEED, "cl.w", (B, 512))).to(_dev())
    labels = torch.tensor([1, 0], device=_dev()) if inst else None
    if keeps == "seeds":
        keeps = (ops.DropSeed(0.75, seed=101), ops.DropSeed(0.75, seed=202), ops.DropSeed(0.75, seed=303) if gate else None)
    elif keeps == "tensors":
        keeps = tuple(((torch.from_numpy(detrand.uniform(SEED, f"cl.keep{i}", (B * N, c))) >= 0.25).float() / 0.75).to(_dev()).to(dtype)
                      for i, c in enumerate((512, 256, 256)))
    for name in off:
        hooks.setattr(functional, name, False)
    if mode == "direct":
        opt = FlatAdam([{"params": list(m.parameters()), "lr": 1e-4}])       # noqa: F841  (owns the gradient buffer)
        assert functional._DIRECT and all(p.grad is not None for p in m.parameters())

    def body():
        if mode == "no_grad":
            with torch.no_grad():
                out = m._run(x, labels, inst, keeps)
            assert not out[0].requires_grad
        else:
            out = m._run(x, labels, inst, keeps)
            ((out[0] * w).sum() + out[3].sum()).backward()
        if result is not None:
            result.update({f"out{i}": o.detach().clone() for i, o in enumerate(out)})
            result.update({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    return _calls(hooks, body)


FORWARD = {
    "fused_gate.no_grad": dict(mode="no_grad", inst=False),
    "fused_gate.inst.no_grad": dict(mode="no_grad"),
}
BACKWARD = {
    "gate_u.eval": dict(),
    "gate_u.eval.noinst": dict(inst=False),
    "gate_u.eval.subtyping_off": dict(subtyping=False),
    "gate_u.eval.group_off": dict(off=("_GROUP_WGRAD",)),
    "gate_u.train": dict(train=True, keeps="seeds"),
    "gate_u.train.group_off": dict(train=True, keeps="seeds", off=("_GROUP_WGRAD",)),
    "gate_u.d256.eval": dict(shape=D256),
    "gate_u.d256.train": dict(shape=D256, train=True, keeps="seeds"),
    "separate.train": dict(train=True, keeps="seeds", off=SEPARATE),
    "injected": dict(train=True, keeps="tensors"),
    "f32.eval": dict(dtype=torch.float32),
    "f32.train.n66": dict(shape=N66, dtype=torch.float32, train=True, keeps="seeds"),
    "plain_attn.f32": dict(dtype=torch.float32, gate=False, train=True, keeps="seeds"),
    "plain_attn.bf16": dict(gate=False, train=True, keeps="seeds"),
    "custom_loss": dict(loss_fn=torch.nn.CrossEntropyLoss(label_smoothing=0.1)),
    "big.gate_u.eval": dict(shape=BIG),
    "big.gate_u.eval.group_off": dict(shape=BIG, off=("_GROUP_WGRAD",)),
    "big.gate_u.train": dict(shape=BIG, train=True, keeps="seeds"),
    "big.gate_u.train.group_off": dict(shape=BIG, train=True, keeps="seeds", off=("_GROUP_WGRAD",)),
    "big.gate_u.custom_loss": dict(shape=BIG, loss_fn=torch.nn.CrossEntropyLoss(label_smoothing=0.1)),
}
CASES = dict(FORWARD)
for _name, _kw in BACKWARD.items():
    CASES[_name + ".plain"] = dict(_kw)
    CASES[_name + ".direct"] = dict(_kw, mode="direct")

RECORDED = {
    "fused_gate.no_grad": [
        "cast_batch", "panel_gemm", "panel_gemm(gate)", "softmax_rows_parts", "weighted_rowsum_acc"
    ],
    "fused_gate.inst.no_grad": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd"
    ],
    "gate_u.eval.plain": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "gate_u.eval.direct": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped",
        "add_lists"
    ],
    "gate_u.eval.noinst.plain": [
        "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "gated_score_bwd_il",
        "gemm_tn_grouped", "panel_gemm", "gemm_tn_grouped"
    ],
    "gate_u.eval.noinst.direct": [
        "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "gated_score_bwd_il",
        "gemm_tn_grouped", "panel_gemm", "gemm_tn_grouped", "add_lists"
    ],
    "gate_u.eval.subtyping_off.plain": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "gate_u.eval.subtyping_off.direct": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped",
        "add_lists"
    ],
    "gate_u.eval.group_off.plain": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "gate_u.eval.group_off.direct": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped",
        "add_lists"
    ],
    "gate_u.train.plain": [
        "cast_batch", "cast_batch", "panel_gemm(drop)", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "gate_u.train.direct": [
        "cast_batch", "cast_batch", "panel_gemm(drop)", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped",
        "add_lists"
    ],
    "gate_u.train.group_off.plain": [
        "cast_batch", "cast_batch", "panel_gemm(drop)", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "gate_u.train.group_off.direct": [
        "cast_batch", "cast_batch", "panel_gemm(drop)", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped",
        "add_lists"
    ],
    "gate_u.d256.eval.plain": [
        "cast_batch", "cast_batch", "gemm_nt", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "relu_bitmask", "panel_gemm", "clam_inst_bwd", "colsum",
        "gemm_tn_grouped"
    ],
    "gate_u.d256.eval.direct": [
        "cast_batch", "cast_batch", "gemm_nt", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "relu_bitmask", "panel_gemm", "clam_inst_bwd", "colsum",
        "gemm_tn_grouped", "add_lists"
    ],
    "gate_u.d256.train.plain": [
        "cast_batch", "cast_batch", "gemm_nt", "dropout_relu_bitmask", "panel_gemm(gate_u)", "softmax_rows_parts",
        "weighted_rowsum_acc", "topk_ids", "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd",
        "colsum", "gemm_tn_grouped"
    ],
    "gate_u.d256.train.direct": [
        "cast_batch", "cast_batch", "gemm_nt", "dropout_relu_bitmask", "panel_gemm(gate_u)", "softmax_rows_parts",
        "weighted_rowsum_acc", "topk_ids", "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd",
        "colsum", "gemm_tn_grouped", "add_lists"
    ],
    "separate.train.plain": [
        "cast_batch", "cast_batch", "panel_gemm", "dropout_relu_bitmask", "cast", "panel_gemm", "gated_score_fwd", "softmax_rows",
        "weighted_rowsum", "topk_ids", "take_rows", "gemm_nt", "cross_entropy", "rows_dot", "softmax_rows_bwd", "gated_score_bwd",
        "gemm_tn_grouped", "transpose_cast", "panel_gemm", "gemm_tn_grouped", "colsum", "gemm_nt_smallk", "scatter_add_rows_masked",
        "colsum", "gemm_tn_grouped"
    ],
    "separate.train.direct": [
        "cast_batch", "cast_batch", "panel_gemm", "dropout_relu_bitmask", "cast", "panel_gemm", "gated_score_fwd", "softmax_rows",
        "weighted_rowsum", "topk_ids", "take_rows", "gemm_nt", "cross_entropy", "rows_dot", "softmax_rows_bwd", "gated_score_bwd",
        "gemm_tn_grouped", "transpose_cast", "panel_gemm", "gemm_tn_grouped", "colsum", "gemm_nt_smallk", "scatter_add_rows_masked",
        "colsum", "gemm_tn_grouped", "add_lists"
    ],
    "injected.plain": [
        "cast_batch", "cast_batch", "panel_gemm", "mul", "cast", "panel_gemm", "gated_score_fwd", "softmax_rows", "weighted_rowsum",
        "topk_ids", "clam_inst_fwd", "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast",
        "relu_bitmask", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "injected.direct": [
        "cast_batch", "cast_batch", "panel_gemm", "mul", "cast", "panel_gemm", "gated_score_fwd", "softmax_rows", "weighted_rowsum",
        "topk_ids", "clam_inst_fwd", "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast",
        "relu_bitmask", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped", "add_lists"
    ],
    "f32.eval.plain": [
        "cast_batch", "gemm_nt", "gemm_nt", "gated_score_fwd", "softmax_rows", "weighted_rowsum", "topk_ids", "clam_inst_fwd",
        "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast", "gemm_nt", "clam_inst_bwd", "colsum",
        "gemm_tn_grouped", "colsum"
    ],
    "f32.eval.direct": [
        "cast_batch", "gemm_nt", "gemm_nt", "gated_score_fwd", "softmax_rows", "weighted_rowsum", "topk_ids", "clam_inst_fwd",
        "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast", "gemm_nt", "clam_inst_bwd", "colsum",
        "gemm_tn_grouped", "colsum", "add_lists"
    ],
    "f32.train.n66.plain": [
        "cast_batch", "gemm_nt", "dropout_mask", "mul", "gemm_nt", "gated_score_fwd", "softmax_rows", "weighted_rowsum", "topk_ids",
        "clam_inst_fwd", "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "clam_inst_bwd", "colsum", "gemm_tn_grouped", "colsum"
    ],
    "f32.train.n66.direct": [
        "cast_batch", "gemm_nt", "dropout_mask", "mul", "gemm_nt", "gated_score_fwd", "softmax_rows", "weighted_rowsum", "topk_ids",
        "clam_inst_fwd", "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "clam_inst_bwd", "colsum", "gemm_tn_grouped", "colsum", "add_lists"
    ],
    "plain_attn.f32.plain": [
        "cast_batch", "gemm_nt", "dropout_relu_bitmask", "gemm_nt", "gated_score_fwd", "softmax_rows", "weighted_rowsum", "topk_ids",
        "clam_inst_fwd", "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "clam_inst_bwd", "colsum", "gemm_tn_grouped", "colsum"
    ],
    "plain_attn.f32.direct": [
        "cast_batch", "gemm_nt", "dropout_relu_bitmask", "gemm_nt", "gated_score_fwd", "softmax_rows", "weighted_rowsum", "topk_ids",
        "clam_inst_fwd", "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "clam_inst_bwd", "colsum", "gemm_tn_grouped", "colsum", "add_lists"
    ],
    "plain_attn.bf16.plain": [
        "cast_batch", "cast", "panel_gemm(drop)", "cast", "panel_gemm", "gated_score_fwd", "softmax_rows", "weighted_rowsum",
        "topk_ids", "clam_inst_fwd", "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "clam_inst_bwd", "colsum", "gemm_tn_grouped", "colsum"
    ],
    "plain_attn.bf16.direct": [
        "cast_batch", "cast", "panel_gemm(drop)", "cast", "panel_gemm", "gated_score_fwd", "softmax_rows", "weighted_rowsum",
        "topk_ids", "clam_inst_fwd", "rows_dot", "softmax_rows_bwd", "gated_score_bwd", "gemm_tn_grouped", "transpose_cast", "gemm_nt",
        "clam_inst_bwd", "colsum", "gemm_tn_grouped", "colsum", "add_lists"
    ],
    "custom_loss.plain": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "take_rows", "gemm_nt", "cross_entropy", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "gemm_tn_grouped", "colsum",
        "gemm_nt_smallk", "scatter_add_rows_masked", "colsum", "gemm_tn_grouped"
    ],
    "custom_loss.direct": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "take_rows", "gemm_nt", "cross_entropy", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "gemm_tn_grouped", "colsum",
        "gemm_nt_smallk", "scatter_add_rows_masked", "colsum", "gemm_tn_grouped", "add_lists"
    ],
    "big.gate_u.eval.plain": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "big.gate_u.eval.direct": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped", "add_lists"
    ],
    "big.gate_u.eval.group_off.plain": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "big.gate_u.eval.group_off.direct": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped",
        "add_lists"
    ],
    "big.gate_u.train.plain": [
        "cast_batch", "cast_batch", "panel_gemm(drop)", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "big.gate_u.train.direct": [
        "cast_batch", "cast_batch", "panel_gemm(drop)", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped", "add_lists"
    ],
    "big.gate_u.train.group_off.plain": [
        "cast_batch", "cast_batch", "panel_gemm(drop)", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped"
    ],
    "big.gate_u.train.group_off.direct": [
        "cast_batch", "cast_batch", "panel_gemm(drop)", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "clam_inst_fwd", "gated_score_bwd_il", "gemm_tn_grouped", "panel_gemm", "clam_inst_bwd", "colsum", "gemm_tn_grouped",
        "add_lists"
    ],
    "big.gate_u.custom_loss.plain": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "take_rows", "gemm_nt", "cross_entropy", "gated_score_bwd_il", "panel_gemm", "gemm_tn_grouped", "colsum", "gemm_nt_smallk",
        "scatter_add_rows_masked", "colsum", "gemm_tn_grouped"
    ],
    "big.gate_u.custom_loss.direct": [
        "cast_batch", "cast_batch", "panel_gemm", "panel_gemm(gate_u)", "softmax_rows_parts", "weighted_rowsum_acc", "topk_ids",
        "take_rows", "gemm_nt", "cross_entropy", "gated_score_bwd_il", "panel_gemm", "gemm_tn_grouped", "colsum", "gemm_nt_smallk",
        "scatter_add_rows_masked", "colsum", "gemm_tn_grouped", "add_lists"
    ],
}


@pytest.mark.parametrize("name", list(CASES))
def test_call_sequence_is_the_recorded_one(name, hooks):
    assert _run(hooks, **CASES[name]) == RECORDED[name]


def test_grouped_plan_by_rows():
    """``murcl_gemm_tn_plan`` (host arithmetic) groups the two weight gradients of the gate_u backward from B*N = 16384 rows on: the
    "big" cases sit on the smallest such shape, every other case below it."""
    import ctypes
    from murcl_amd import _lib, ops

    def grouped(rows):
        arr, kinds = (_lib.TnProblem * 2)(), (ctypes.c_int * 2)()
        arr[0] = arr[1] = _lib.TnProblem(None, None, None, None, None, rows, 512, 512, 512, 512, 512, 0, 0, 1.0)
        return _lib.lib().murcl_gemm_tn_plan(arr, 2, _lib.BF16, kinds) >= 0 and ops._tn_sq_group(list(kinds))
    assert grouped(BIG[0] * BIG[1]) and not any(grouped(rows) for rows in range(32, BIG[0] * BIG[1], 32))


def test_route_by_shape():
    """The cases above take the routes their names say (and the bench shape the gate_u route): (first layer by the panel kernel, its
    epilogue leaves the bit mask, Dropout form, gate form, panel dz1 product, one-launch instance branch)."""
    from murcl_amd.functional import clam_route
    bf16, f32, inst = torch.bfloat16, torch.float32, (2, 8, False)
    assert clam_route(2, 64, 512, 512, 256, bf16, True, None, False, False, inst) == (True, False, None, "fused", False, True)
    assert clam_route(2, 64, 512, 512, 256, bf16, True, None, True, True, inst) == (True, True, None, "u", True, True)
    assert clam_route(2, 64, 512, 512, 256, bf16, True, "seeds", True, True, inst) == \
        clam_route(64, 4096, 512, 512, 256, bf16, True, "seeds", True, True, inst) == (True, True, "epilogue", "u", True, True)
    assert clam_route(2, 64, 256, 512, 256, bf16, True, "seeds", True, True, inst) == (False, False, "bitmask", "u", True, True)
    assert clam_route(2, 64, 512, 512, 256, bf16, True, "tensors", True, True, inst) == (True, False, "injected", "panel", True, True)
    assert clam_route(2, 66, 512, 512, 256, f32, True, "seeds", True, True, inst) == (False, False, "mask", "tile", False, True)
    assert clam_route(2, 64, 512, 512, 256, bf16, False, "seeds", True, True, inst) == (True, True, "epilogue", "panel", False, True)
    assert clam_route(2, 64, 512, 512, 256, bf16, True, None, True, True, (2, 8, True)).inst_fused is False
