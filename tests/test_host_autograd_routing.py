"""Direct gradient accumulation follows what autograd was asked for (host only, no GPU).

``functional._direct(p)`` decides whether a backward kernel adds p's gradient into the pre-seated ``p.grad`` itself (and hands
autograd None).  That is only right when the running backward pass would accumulate into ``p.grad`` anyway: under
``backward(inputs=[x])`` or ``autograd.grad(...)`` the parameter's ``.grad`` must stay as it was.
"""
import pytest
import torch

from murcl_amd import functional


class _Probe(torch.autograd.Function):
    """y = x * p; records ``_direct(p)`` (twice: the second answer comes from the per-pass cache) during its backward.  ``prime``:
    the backward starts with ``functional._enter(ctx)`` (answers from the node's own edges) as the library's Functions do;
    otherwise ``_direct`` looks the accumulator up itself."""
    seen = []
    prime = False

    @staticmethod
    def forward(ctx, x, p):
        ctx.save_for_backward(x, p)
        return x * p

    @staticmethod
    def backward(ctx, g):
        if _Probe.prime:
            functional._enter(ctx)
        x, p = ctx.saved_tensors
        _Probe.seen.append((functional._direct(p), functional._direct(p)))
        return g * p, g * x


@pytest.fixture(params=[False, True], ids=["lookup", "primed"])
def direct(monkeypatch, request):
    monkeypatch.setattr(functional, "_DIRECT", True)
    monkeypatch.setattr(_Probe, "prime", request.param)
    _Probe.seen = []
    x = torch.randn(5, requires_grad=True)
    p = torch.nn.Parameter(torch.randn(5))
    p.grad = torch.zeros_like(p)                        # pre-seated f32 buffer, as FlatAdam leaves it
    return x, p


ROUTES = {
    "backward": (lambda y, x, p: y.backward(), True),
    "backward_inputs_x": (lambda y, x, p: y.backward(inputs=[x]), False),
    "grad_x": (lambda y, x, p: torch.autograd.grad(y, [x]), False),
    "grad_p": (lambda y, x, p: torch.autograd.grad(y, [p]), False),
    "grad_x_p": (lambda y, x, p: torch.autograd.grad(y, [x, p]), False),
    "backward_inputs_p": (lambda y, x, p: y.backward(inputs=[p]), True),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_direct_only_where_the_engine_accumulates_into_the_parameter(direct, route):
    x, p = direct
    run, want = ROUTES[route]
    run(_Probe.apply(x, p).sum(), x, p)
    assert _Probe.seen == [(want, want)]


def test_direct_answer_is_per_backward_pass(direct):
    """The cached answer of one pass does not leak into the next (partial, full, partial in a row)."""
    x, p = direct
    for run, want in (ROUTES["grad_x"], ROUTES["backward"], ROUTES["backward_inputs_x"], ROUTES["backward"]):
        run(_Probe.apply(x, p).sum(), x, p)
        assert _Probe.seen[-1] == (want, want)


def test_direct_needs_the_mode_and_a_seated_buffer(direct, monkeypatch):
    x, p = direct
    assert not functional._direct(p)                     # outside a backward pass nothing accumulates
    p.grad = None
    _Probe.apply(x, p).sum().backward()
    assert _Probe.seen[-1] == (False, False)
    p.grad = torch.zeros_like(p)
    monkeypatch.setattr(functional, "_DIRECT", False)
    _Probe.apply(x, p).sum().backward()
    assert _Probe.seen[-1] == (False, False)
