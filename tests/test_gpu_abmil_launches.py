"""The launches of one ABMIL forward + backward, per configuration, as the sequence of ``ops.TIMERS`` span keys.

``functional._abmil_backward`` serves the default configuration, the general one (dropout, other L / D) and the ``EncoderSession``;
the bf16 fast forward chain serves ``ABMILFn`` and ``ABMILStepFn``.  The sequences below were recorded with the same recorder from
the code that spelled these paths out separately (commit 417effe), so they pin what the shared functions must launch: exactly, in
order, on the default / f32 512-128 / session paths; on the general paths the encoder weight gradients (the ``gemm_tn*`` keys) may
sit anywhere - the same launches, and everything else in order.  (A span key names the kernel family and its shape class, not the
operands: the gradient assertions of test_gpu_modules.py / test_gpu_autograd_contract.py / test_gpu_step.py hold the numbers.)

Second part: the CU budget of the overlapped backward launches (``functional._overlap_budget``) is restored when a launch inside
its scope raises.
"""
import pytest
import torch

from oracle import params as P

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SEED = 29

# the smallest default-shape batch the bf16 fast path takes with more than one bag (abmil_fast_path: N % 32 == 0; the pooling
# kernels accept N = 128)
B0, N0 = 2, 128
# the G16 shapes of tests/test_gpu_modules.py (oracle/recipes.py): 3 bags x 160 patches; "small" = d 320, L 256, D 64
BG, NG = 3, 160


class _Recorder:
    """Stands in for an ``ops.KernelTimers``: every span key in launch order, nothing timed."""

    def __init__(self):
        self.keys = []

    def span(self, key, work=None):
        from murcl_amd import ops
        self.keys.append(key)
        return ops._NULL


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dtype, d=512, L=512, D=128, dropout=0.0):
    from murcl_amd.models.abmil import ABMIL
    m = ABMIL(d, L=L, D=D, dim_out=2, dropout=dropout)
    m.load_state_dict(P.to_torch(P.abmil(SEED, dim_in=d, L=L, D=D, dim_out=2)))
    m.compute_dtype = dtype
    return m.to(_dev()).train()


def _bags(tag, B, N, d, dtype):
    return torch.from_numpy(P.bags(SEED, f"launches.{tag}", B, N, d)).to(_dev()).to(dtype)


@pytest.fixture
def hooks(monkeypatch):
    """Every module-level switch of functional.py at its default, whatever an earlier test of the process left behind."""
    from murcl_amd import functional
    for name, value in [("_DIRECT", False), ("_MILESTONE", None), ("_GROUP_WGRAD", True), ("_FOLD_BIAS", True), ("_FRAG_WEIGHTS", True),
                        ("_STREAM_A", 4), ("_DEFER_ON", True), ("_DEFERRED", None), ("_OVERLAP_BUDGET", None)]:
        monkeypatch.setattr(functional, name, value)
    return monkeypatch


def _record(hooks, run):
    from murcl_amd import ops
    rec = _Recorder()
    hooks.setattr(ops, "TIMERS", rec)
    run(rec)
    torch.cuda.synchronize()
    hooks.setattr(ops, "TIMERS", None)
    return rec.keys


def _fwd_bwd(m, x):
    out, _ = m(x)
    out.sum().backward()


def _seat(m):
    """Direct gradient accumulation as the training loops run it: a FlatAdam seats every ``.grad`` in its flat buffer."""
    from murcl_amd import functional
    from murcl_amd.optim import FlatAdam
    opt = FlatAdam([{"params": list(m.parameters()), "lr": 1e-4}])
    assert functional._DIRECT and all(p.grad is not None for p in m.parameters())
    return opt


def run_bf16_default(hooks):
    m, x = _model(BF16), _bags("default", B0, N0, 512, BF16).requires_grad_()       # (with the input gradient)
    return _record(hooks, lambda rec: _fwd_bwd(m, x))


def run_bf16_direct(hooks):
    m, x = _model(BF16), _bags("default", B0, N0, 512, BF16)
    opt = _seat(m)                                                                   # noqa: F841  (owns the gradient buffer)
    return _record(hooks, lambda rec: _fwd_bwd(m, x))


def run_bf16_ungrouped(hooks):
    from murcl_amd import functional
    hooks.setattr(functional, "_GROUP_WGRAD", False)
    return run_bf16_direct(hooks)


def run_bf16_milestone(hooks):
    """Per-layer milestones (a data-parallel reducer): the ungrouped order, the callbacks between the launches."""
    from murcl_amd import functional
    m, x = _model(BF16), _bags("default", B0, N0, 512, BF16)
    opt = _seat(m)                                                                   # noqa: F841

    def run(rec):
        hooks.setattr(functional, "_MILESTONE", lambda params: rec.keys.append(f"milestone({len(params)})"))
        _fwd_bwd(m, x)
    return _record(hooks, run)


def run_bf16_dropout(hooks):
    from murcl_amd import ops
    m, x = _model(BF16, dropout=0.25), _bags("dropout", BG, NG, 512, BF16)
    m.keep_masks = (ops.DropSeed(0.75, seed=1234567), ops.DropSeed(0.75, seed=7654321))
    return _record(hooks, lambda rec: _fwd_bwd(m, x))


def run_f32_default(hooks):
    m, x = _model(F32), _bags("default", B0, N0, 512, F32)
    return _record(hooks, lambda rec: _fwd_bwd(m, x))


def run_f32_generic(hooks):
    m, x = _model(F32, d=320, L=256, D=64), _bags("small", BG, NG, 320, F32)
    return _record(hooks, lambda rec: _fwd_bwd(m, x))


def run_session(hooks):
    from murcl_amd import functional
    m = _model(BF16)
    xs = [_bags(f"session{t}", B0, N0, 512, BF16) for t in range(2)]
    opt = _seat(m)                                                                   # noqa: F841

    def run(rec):
        m.session = functional.EncoderSession(2, B0, N0, 512, 512, BF16, _dev())
        try:
            outs = [m(x)[0] for x in xs]
            (outs[0].sum() + outs[1].sum()).backward()
        finally:
            m.session = None
    return _record(hooks, run)


EXACT = {
    "bf16_default": (run_bf16_default, [
        "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "row:k2_fwd<bf16>",
        "abmil_pool_fwd<bf16>", "abmil_pool_decoder", "gemm_nt<f32,f32,NONE>", "abmil_pool_bwd<bf16>", "gemm_tn<bf16>",
        "panel_gemm<K128,RANK1_MASK>", "panel_gemm<K512,MASK>", "panel_gemm<K512,MASK>", "gemm_tn<bf16>",
        "gemm_nt<bf16,bf16,NONE>",
    ]),
    "bf16_direct": (run_bf16_direct, [
        "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "row:k2_fwd<bf16>",
        "abmil_pool_fwd<bf16>", "abmil_pool_decoder", "gemm_tn<f32>", "gemm_nt<f32,f32,NONE>", "abmil_pool_bwd<bf16>",
        "gemm_tn<bf16>", "panel_gemm<K128,RANK1_MASK>", "panel_gemm<K512,MASK>", "panel_gemm<K512,MASK>", "gemm_tn<bf16>",
    ]),
    "bf16_ungrouped": (run_bf16_ungrouped, [
        "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "row:k2_fwd<bf16>",
        "abmil_pool_fwd<bf16>", "abmil_pool_decoder", "gemm_tn<f32>", "gemm_nt<f32,f32,NONE>", "abmil_pool_bwd<bf16>",
        "gemm_tn<bf16>", "panel_gemm<K128,RANK1_MASK>", "gemm_tn<bf16>", "panel_gemm<K512,MASK>", "gemm_tn<bf16>",
        "panel_gemm<K512,MASK>", "gemm_tn<bf16>",
    ]),
    "bf16_milestone": (run_bf16_milestone, [
        "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "row:k2_fwd<bf16>",
        "abmil_pool_fwd<bf16>", "abmil_pool_decoder", "gemm_tn<f32>", "gemm_nt<f32,f32,NONE>", "abmil_pool_bwd<bf16>",
        "gemm_tn<bf16>", "milestone(6)", "panel_gemm<K128,RANK1_MASK>", "gemm_tn<bf16>", "milestone(2)", "panel_gemm<K512,MASK>",
        "gemm_tn<bf16>", "milestone(2)", "panel_gemm<K512,MASK>", "gemm_tn<bf16>",
    ]),
    "f32_default": (run_f32_default, [
        "gemm_nt<f32,f32,BIAS_RELU>", "gemm_nt<f32,f32,BIAS_RELU>", "gemm_nt<f32,f32,BIAS_RELU>", "row:k2_fwd<f32>",
        "abmil_pool_fwd<f32>", "abmil_pool_decoder", "gemm_nt<f32,f32,NONE>", "abmil_pool_bwd<f32>",
        "gemm_nt<f32,f32,RANK1_MASK>", "gemm_nt<f32,f32,MASK>", "gemm_nt<f32,f32,MASK>",
    ]),
    "session": (run_session, [
        "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "row:k2_fwd<bf16>",
        "abmil_pool_fwd<bf16>", "abmil_pool_decoder", "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>",
        "panel_gemm<K512,BIAS_RELU>", "row:k2_fwd<bf16>", "abmil_pool_fwd<bf16>", "abmil_pool_decoder", "gemm_tn<f32>",
        "gemm_nt<f32,f32,NONE>", "abmil_pool_bwd<bf16>", "gemm_tn<bf16>", "panel_gemm<K128,RANK1_MASK>", "panel_gemm<K512,MASK>",
        "panel_gemm<K512,MASK>", "gemm_tn<bf16>",
    ]),
}

GENERAL = {
    "bf16_dropout": (run_bf16_dropout, [
        "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "panel_gemm<K512,BIAS_RELU>", "row:k2_fwd<bf16>",
        "abmil_pool_fwd<bf16>", "abmil_pool_decoder", "gemm_nt<f32,f32,NONE>", "abmil_pool_bwd<bf16>", "gemm_tn<bf16>",
        "panel_gemm<K128,RANK1_MASK>", "panel_gemm<K512,MASK>", "panel_gemm<K512,MASK>", "gemm_tn<bf16>", "gemm_tn<bf16>",
        "gemm_tn<bf16>",
    ]),
    "f32_generic": (run_f32_generic, [
        "gemm_nt<f32,f32,BIAS_RELU>", "gemm_nt<f32,f32,BIAS_RELU>", "gemm_nt<f32,f32,BIAS_RELU>", "gemm_nt<f32,f32,BIAS>",
        "weighted_rowsum<f32>", "gemm_nt<f32,f32,BIAS_RELU>", "gemm_nt<f32,f32,NONE>", "rows_dot<f32>",
        "gemm_nt<f32,f32,RANK1_MASK>", "gemm_nt<f32,f32,MASK>", "gemm_nt<f32,f32,MASK>",
    ]),
}


@pytest.mark.parametrize("name", list(EXACT))
def test_launch_sequence_is_the_recorded_one(name, hooks):
    run, want = EXACT[name]
    got = run(hooks)
    assert got == want


@pytest.mark.parametrize("name", list(GENERAL))
def test_general_path_launches_are_the_recorded_ones(name, hooks):
    """The same launches, and all but the encoder weight gradients in the recorded order."""
    run, want = GENERAL[name]
    got = run(hooks)
    rest = lambda keys: [k for k in keys if not k.startswith("gemm_tn")]      # noqa: E731
    assert rest(got) == rest(want)
    assert sorted(got) == sorted(want)


def test_overlap_budget_is_restored_when_a_launch_inside_raises(hooks):
    """A host-side error between the pooling backward and the last input gradient must not leave the reduced CU budget in force
    for the rest of the process."""
    from murcl_amd import functional, ops
    m, x = _model(BF16), _bags("default", B0, N0, 512, BF16)
    out, _ = m(x)
    before = ops.cu_budget()
    hooks.setattr(functional, "_OVERLAP_BUDGET", before // 2)

    def refuse(*a, **k):
        raise RuntimeError("refused on the host")
    hooks.setattr(ops, "panel_gemm", refuse)                     # the first input gradient of the backward pass: inside the scope
    try:
        with pytest.raises(RuntimeError, match="refused on the host"):
            out.sum().backward()
        after = ops.cu_budget()
    finally:
        ops.set_cu_budget(before)
    assert after == before
