"""autograd.Functions that stitch the HIP kernels into differentiable ops.

Forward and backward are sequences of C-ABI launches (murcl_amd.ops); torch supplies
only tensor storage and the autograd graph.  No CPU / eager-PyTorch fallback exists:
CPU tensors raise.
"""
import collections
import contextlib
import functools
import math

import torch

from . import ops


def _flat2(x):
    return x.reshape(-1, x.shape[-1])


# Direct gradient accumulation.  With FlatAdam every parameter's ``.grad`` is a zeroed view of one flat buffer before
# the backward pass starts, so the weight-gradient GEMM / column-sum kernels can add into it themselves (their split-M
# reduction accumulates into the output anyway) and hand autograd ``None``: no zero-filled temporary and no
# AccumulateGrad add per parameter.  Opt-in because it bypasses per-parameter autograd hooks.
_DIRECT = False


def set_direct_grad(flag):
    """Enable/disable accumulation of parameter gradients straight into pre-seated ``.grad`` buffers."""
    global _DIRECT
    _DIRECT = bool(flag)


_MILESTONE = None
# bit l -> encoder layer l+1 loads its input with the non-temporal policy.  Layer 3's input (H2) is not read again before
# the backward pass, while its output (H3) is what the pooling kernel streams next: kept out of the Infinity Cache, H2
# leaves more of H3 there (K2 forward 67.6 -> 62.4 us inside the step; the other layers measured neutral-to-slower).
_STREAM_A = 4
# Which of two BUILT forms a call takes where both cover its shape.  The right-hand side of each line is the form every default
# configuration runs; the other one is the general chain that shapes outside the fused kernels' reach take anyway (other widths,
# more classes, per-layer gradient milestones ...), so both stay tested: the parity tests flip these through monkeypatch
# (tests/test_gpu_modules.py) - they are test hooks, not environment switches (round 5: the MURCL_* variables are gone).
_FUSED_GATE = True        # CLAM, forward-only calls: the gate score from the gate GEMM's epilogue, no [B*N, 2D] pre-activations
_GATE_U = True            # CLAM, training chain: score + pre-activations from one gate GEMM, one-pass gate backward
_FUSED_FC_DROP = True     # CLAM: the seeded Dropout behind the first layer's ReLU inside that GEMM's epilogue
_FUSED_INST = True        # CLAM: the instance branch as one launch forward, one backward
_GROUP_WGRAD = True       # the encoder weight gradients of a backward pass as one grouped launch
_FOLD_BIAS = True         # encoder bias gradients folded into the wgrad reduce
_FRAG_WEIGHTS = True      # ABMIL bf16 fast path: the K = 512 weight operands as FRAGMENT-ORDER views (ops.is_frag; round 6)


def _frag_specs(w1, w2, w3, wa, T):
    """The seven weight views of the bf16 ABMIL chain with every K = 512 operand in fragment order: W1..W3, Wa (forward, pooling) and
    W3^T, W2^T (the masked input gradients); Wa^T [512,128] (the rank-1 input gradient, K = 128) stays row-major."""
    return [(w1, False, T, "frag"), (w2, False, T, "frag"), (w3, False, T, "frag"), (wa, False, T, "frag"),
            (wa, True, T), (w3, True, T, "frag"), (w2, True, T, "frag")]


# CUs the launches of the aggregator's backward pass - pooling backward up to the last input gradient - are sized for while a
# collective may be running beside them (None: ops.cu_budget() as it is).  The head group's gradient all-reduce is launched when
# backward reaches the aggregator outputs (dist.OverlappedGradReduce) and is in flight for roughly these launches (19.4 MB at the
# xGMI ring's ~150 GB/s = 0.2-0.3 ms against 65 + 65 + 82 + 2 x 133 us); the forward pass, the grouped weight gradients behind them
# and the optimizer run with no collective beside them and keep the full chip.
_OVERLAP_BUDGET = None


def set_overlap_cu_budget(cus):
    """``cus`` (or None) = the CU budget in force for the backward launches a gradient all-reduce overlaps."""
    global _OVERLAP_BUDGET
    _OVERLAP_BUDGET = None if cus is None else int(cus)


class _overlap_budget:
    """Context: the persistent launches inside are sized for ``_OVERLAP_BUDGET`` CUs (murcl_set_cu_budget), the budget that was
    in force before is restored on exit.  Launchers read the budget when they enqueue, so this is host-side bookkeeping only."""

    def __enter__(self):
        self.prev = None
        if _OVERLAP_BUDGET is not None:
            self.prev = ops.cu_budget()
            ops.set_cu_budget(min(self.prev, _OVERLAP_BUDGET))
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            ops.set_cu_budget(self.prev)
        return False


def set_grad_milestone(callback):
    """``callback(params)`` is called from inside the aggregator's backward as soon as the kernels that complete the
    gradients of ``params`` are enqueued (direct-gradient mode only).  A data-parallel reducer uses it to start their
    all-reduce under the remaining backward kernels; only meaningful when the aggregator runs once per optimizer step."""
    global _MILESTONE
    _MILESTONE = callback


def _final(*params):
    if _MILESTONE is not None and all(_direct(p) for p in params):
        _MILESTONE(params)


def _direct(p):
    """Does this backward pass add p's gradient into its pre-seated ``.grad`` itself (and hand autograd None)?  Only in direct mode,
    for a leaf whose ``.grad`` is a contiguous f32 buffer, and only when the pass accumulates into p at all: ``backward(inputs=[x])``
    and ``autograd.grad(loss, [x])`` leave p's AccumulateGrad node out, ``autograd.grad(loss, [p])`` hands p's gradient back instead
    (the engine's query raises for a leaf it captures).  One answer per parameter and backward pass (graph task), not one per call:
    ``_enter(ctx)`` at the top of a backward answers for the Function's own leaf inputs from its graph edges; a parameter it did not
    cover is looked up through its gradient edge (a view op to reach the accumulator node)."""
    if not _DIRECT or p is None:
        return False
    if torch._C._current_graph_task_id() != _ACC_TASK:
        _new_task()
    hit = _ACC.get(id(p))
    if hit is None:
        hit = _ACC[id(p)] = _seated(p) and _will_execute(torch.autograd.graph.get_gradient_edge(p).node)
    return hit


# (non-leaf tensors - a row of ``attention.2`` handed to one head of ABMIL(K > 1) - have no pre-seated gradient)
def _seated(p):
    return p.is_leaf and p.requires_grad and p.grad is not None and p.grad.is_contiguous() and p.grad.dtype == torch.float32


_ACC_TASK, _ACC = -1, {}
_ACC_NODE = torch._C._functions.AccumulateGrad


def _new_task():
    global _ACC_TASK
    _ACC_TASK = torch._C._current_graph_task_id()
    _ACC.clear()


def _will_execute(node):
    try:
        return torch._C._will_engine_execute_node(node)
    except RuntimeError:
        return False


def _enter(ctx):
    """Called first by a backward that may accumulate directly: the ``_direct`` answers for every leaf input of the Function."""
    if not _DIRECT:
        return
    if torch._C._current_graph_task_id() != _ACC_TASK:
        _new_task()
    for fn, _ in ctx.next_functions:
        if type(fn) is _ACC_NODE:
            v = fn.variable
            if id(v) not in _ACC:
                _ACC[id(v)] = _seated(v) and _will_execute(fn)


# Which parameters received a gradient since their optimizer last stepped.  torch.optim.Adam skips parameters whose
# ``.grad`` is None (never reached by backward: ABMIL.fc, CLAM's classifiers in pre-training, DSMIL's fcc): no weight
# decay, no moment update, no step count.  With pre-seated zeroed gradient views "never reached" is invisible in the
# buffer, so every writer announces itself here: the direct-accumulation helpers below, and an autograd
# post-accumulate hook that FlatAdam registers for gradients that arrive through AccumulateGrad.
_TOUCHED = set()


def _touch(*params):
    for p in params:
        if p is not None:
            _TOUCHED.add(id(p))


def _wgrad(dy, x, w, b=None, bias_parts=None):
    """dW = dy^T x [N1,N2]; returns it, or adds it to w.grad and returns None.  ``bias_parts`` (direct mode only): the
    partial column-sum rows of dy that the kernel which produced dy left behind - the bias gradient, added to b.grad by
    the same launches."""
    if _direct(w):
        if bias_parts is not None:
            ops.gemm_tn(dy, x, out=w.grad, colsum_into=b.grad.view(-1), colsum_parts=bias_parts)
            _touch(w, b)
        else:
            ops.gemm_tn(dy, x, out=w.grad)
            _touch(w)
        return None
    assert bias_parts is None
    return ops.gemm_tn(dy, x)


def _wgrad_group(items):
    """[(dy, x, w, b, bias_parts)] -> [dW or None]: ``_wgrad`` for several layers in one grouped launch (``ops.gemm_tn_grouped``)."""
    probs = []
    for dy, x, w, b, parts in items:
        if _direct(w):
            probs.append((dy, x, w.grad, b.grad.view(-1) if parts is not None else None, parts))
            _touch(w)
            if parts is not None:
                _touch(b)
        else:
            assert parts is None
            probs.append((dy, x, None, None, None))
    Cs = ops.gemm_tn_grouped(probs, fresh=True)           # (products without a pre-seated gradient are written, not accumulated: no fill)
    return [None if _direct(it[2]) else C for it, C in zip(items, Cs)]


# Deferred weight gradients.  A recurrent head that is stepped T times per optimizer step (the MuRCL loop: T patch steps
# through ONE Full_layer) produces T weight gradients per parameter, each a skinny [128 x N]^T [128 x K] product whose
# [N x K] f32 output leaves as float atomics (6.3 MB for W_ih, 12.6 MB for W_hh - 15 us apiece, T times).  Inside a
# ``deferred_wgrads()`` block the (dy, x) pairs are only queued; on exit each parameter gets ONE product over the
# concatenated T*128 rows: the same sum, one launch and one pass of atomics instead of T.
_DEFERRED = None
_DEFER_ON = True           # test hook (see the list at the top)


class deferred_wgrads:
    def __enter__(self):
        global _DEFERRED
        self.prev, _DEFERRED = _DEFERRED, ({} if _DEFER_ON else None)
        return self

    def __exit__(self, *exc):
        global _DEFERRED
        queue, _DEFERRED = _DEFERRED, self.prev
        if exc[0] is None and queue:
            _flush(queue)
        return False


def _flush(queue):
    """The queued (dy, x) pairs of every parameter as one product each, up to four small f32 products per launch."""
    probs = []
    for w, b, dys, xs in queue.values():
        dy = dys[0] if len(dys) == 1 else torch.cat(dys, 0)
        x = xs[0] if len(xs) == 1 else torch.cat(xs, 0)
        probs.append((dy, x, w.grad, b.grad.view(-1) if b is not None else None, None))
    queue.clear()
    for i in range(0, len(probs), 4):
        ops.gemm_tn_grouped(probs[i:i + 4])


def flush_deferred():
    """Run what the active ``deferred_wgrads`` block has queued so far (a gradient all-reduce that starts inside the backward pass
    needs the gradients of the layers behind it complete: dist.OverlappedGradReduce)."""
    if _DEFERRED:
        _flush(_DEFERRED)


def _defer(dy, x, w, b):
    """Queue (dy, x) for w (and b) when a deferral block is active and both accumulate directly; True if queued."""
    if _DEFERRED is None or not _direct(w) or (b is not None and not _direct(b)):
        return False
    ent = _DEFERRED.get(id(w))
    if ent is None:
        ent = _DEFERRED[id(w)] = (w, b, [], [])
    elif (ent[1] is None) != (b is None):
        return False
    ent[2].append(dy)
    ent[3].append(x)
    _touch(w, b)
    return True


def _wbgrad(dy, x, w, b):
    """(dW, db) of one Linear; in direct mode both are added to the flat gradient buffer by ONE launch."""
    if _defer(dy, x, w, b):
        return None, None
    if _direct(w) and _direct(b):
        ops.gemm_tn(dy, x, out=w.grad, colsum_into=b.grad.view(-1))
        _touch(w, b)
        return None, None
    return _wgrad(dy, x, w), _bgrad(dy, b)


def _bgrad(dy, b):
    """db = column sums of dy."""
    if _direct(b):
        ops.colsum(dy, out=b.grad.view(-1), accumulate=True)
        _touch(b)
        return None
    return ops.colsum(dy)


def _pgrads(*pairs):
    """``[(gradient tensor or None, parameter)]`` -> the list of what autograd should still see: parameters that accumulate directly
    get their gradients added to the pre-seated buffers by ONE launch for all of them (and None here), the others get theirs back."""
    direct = [(g, p) for g, p in pairs if g is not None and _direct(p)]
    if len(direct) > 1:
        ops.add_lists([(g.reshape(p.grad.shape) if g.shape != p.grad.shape else g, p.grad) for g, p in direct])
        _touch(*(p for _, p in direct))
        done = {id(p) for _, p in direct}
        return [None if (g is None or id(p) in done) else g for g, p in pairs]
    return [g for g, _ in pairs]


def _pgrad(g, p):
    """A gradient that a kernel already produced as its own tensor."""
    if _direct(p):
        p.grad.add_(g.view_as(p.grad))
        _touch(p)
        return None
    return g


class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b) for small (bag-level) f32 matrices; act in {none, relu}."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        x2 = _flat2(x).contiguous()
        y = ops.gemm_nt(x2, w, epi=ops.EPI_BIAS_RELU if relu else ops.EPI_BIAS, bias=b)
        ctx.save_for_backward(x2, w, y if relu else None, b)
        ctx.relu = relu
        ctx.xshape = x.shape
        return y if x.dim() == 2 else y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        _enter(ctx)
        x2, w, y, b = ctx.saved_tensors
        dy2 = _flat2(dy).contiguous()
        if ctx.relu:
            dy2 = ops.relu_bwd(dy2, y)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm_nt(dy2, ops.transposed(w)).view(ctx.xshape)
        if ctx.needs_input_grad[1] and ctx.needs_input_grad[2]:
            dw, db = _wbgrad(dy2, x2, w, b)
        else:
            if ctx.needs_input_grad[1]:
                dw = _wgrad(dy2, x2, w)
            if ctx.needs_input_grad[2]:
                db = _bgrad(dy2, b)
        return dx, dw, db, None


def _dropout(h, k, bits):
    """Dropout after a ReLU, in place: h *= keep for ``k`` = a DropSeed or a materialised keep-multiplier tensor.  -> the 1-bit mask
    of the surviving positive entries when ``bits`` (bf16 fast path), else None."""
    seeded = isinstance(k, ops.DropSeed)
    if seeded and h.shape[0] % 32 == 0 and h.shape[1] % 128 == 0:
        return ops.dropout_relu_bitmask(h, k, want_bits=bits)
    ops.mul(h, ops.dropout_mask(h.shape, h.dtype, k.keep_p, h.device, seed=k.seed) if seeded else k.to(h.dtype).reshape(h.shape))
    return ops.relu_bitmask(h) if bits else None


def _abmil_fast_forward(x2, B, N, params, *, views=None, bits=True, drops=None, blocks=None):
    """The bf16 fast chain of ``ABMILFn`` and ``ABMILStepFn`` (shapes ``abmil_fast_path`` accepts): three weight-stationary encoder
    GEMMs that also emit 1-bit ReLU masks, the one-pass pooling kernel, the decoder.  ``views``: the seven weight views when the
    caller had to make them itself; ``bits``: write the masks (a backward pass can follow); ``drops``: as ``ABMILFn.forward``;
    ``blocks`` = (h1, h2, h3, m1, m2, m3, scores, (out, M, ml)): caller-owned result buffers (``EncoderSession``).
    -> (h1, h2, h3, m1, m2, m3, scores, M, ml, out, views)"""
    w1, b1, w2, b2, w3, b3, wa, ba, wb, bb, wd, bd = params
    T = x2.dtype
    if views is None:
        # compute-dtype copies of W1..W3, Wa for this pass and W2^T, W3^T, Wa^T for the dgrads of the backward pass: one
        # launch, and only when a parameter changed since they were last built (ops.weight_views)
        views = ops.weight_views(_frag_specs(w1, w2, w3, wa, T) if _FRAG_WEIGHTS else
                                 [(w, False, T) for w in (w1, w2, w3, wa)] + [(wa, True, T), (w3, True, T), (w2, True, T)])
    w1c, w2c, w3c, wac = views[:4]
    o1, o2, o3, bm1, bm2, bm3, sc, triple = blocks or (None,) * 8
    nt = _STREAM_A
    own = bits and drops is None                 # with Dropout the pass that applies it writes the mask of what survives
    h1, m1, _ = ops.panel_gemm(x2, w1c, ops.PG_BIAS_RELU, bias=b1, want_bitmask=own, stream_a=bool(nt & 1), out=o1, bitmask_out=bm1)
    if drops is not None:
        m1 = _dropout(h1, drops[0], bits)
    # layer 2 walks the rows backwards (layer 1 has just written the high rows of h1), layer 3 forwards again,
    # and the pooling kernel backwards: every pass starts on what its producer left in the Infinity Cache
    h2, m2, _ = ops.panel_gemm(h1, w2c, ops.PG_BIAS_RELU, bias=b2, want_bitmask=own, reverse=True, stream_a=bool(nt & 2),
                               out=o2, bitmask_out=bm2)
    if drops is not None:
        m2 = _dropout(h2, drops[1], bits)
    h3, m3, _ = ops.panel_gemm(h2, w3c, ops.PG_BIAS_RELU, bias=b3, want_bitmask=bits, stream_a=bool(nt & 4), out=o3, bitmask_out=bm3)
    # ONE launch for the K2 row (scores + chunk partials); the per-bag merge is part of the decoder launch below and the
    # normalised attention row is formed by the backward pass (or on demand: ``attention_rows``)
    scores, part = ops.abmil_pool_partials(h3.view(B, N, h3.shape[1]), wac, ba, wb, bb, scores=sc)
    out, M, ml = ops.abmil_pool_decoder(part, B, N, T, wd, bd, out=triple)
    return h1, h2, h3, m1, m2, m3, scores, M, ml, out, views


def _abmil_backward(saved, dims, dout, need_dx, wfrag, *, pool_fast, drop_scale):
    """The aggregator's backward pass on explicit tensors: ``ABMILFn.backward`` hands it one call's saved tensors, ``EncoderSession``
    the activations of all patch steps of a training step as one batch.  ``wfrag``: wac, w3t and w2t are fragment-order views
    (``ops.is_frag`` of the forward's views).  ``pool_fast`` / ``drop_scale``: as ``ABMILFn.forward`` left them on ctx.
    -> (dx, dw1, db1, dw2, db2, dw3, db3, dwa, dba, dwb, dbb, dwd, dbd)"""
    (x2, h1, h2, h3, scores, A, M, ml, out, w1, w2, w3, wa, ba, wb, wd, wac, m1, m2, m3,
     b1, b2, b3, bb, bd, wat, w3t, w2t) = saved
    B, N, d = dims
    T = x2.dtype
    L = h3.shape[1]
    panel = m3 is not None           # the bf16 fast chain (so ``pool_fast``: abmil_fast_path): bit-mask panel dgrads; else row-major GEMMs
    # Where each gradient goes.  The tuned default (no dropout, L = 512, D = 128) lets the routing helpers add into pre-seated
    # ``.grad`` buffers, defer and fire milestones.  The other configurations (``--dropout`` > 0 while training, other ``--L`` /
    # ``--D``) get every gradient back as its own tensor - the dropout factors are applied to them at the end: with None in the
    # parameter's place the same helpers neither accumulate (``_direct(None)`` is False), defer, nor fire.
    default = pool_fast and drop_scale is None
    pw1, pb1, pw2, pb2, pw3, pb3, pwa, pba, pwb, pbb, pwd, pbd = \
        (w1, b1, w2, b2, w3, b3, wa, ba, wb, bb, wd, bd) if default else (None,) * 12
    # the three encoder weight gradients wait until the last input gradient exists and run as ONE grouped launch (one round of
    # workgroups, one reduce launch: ops.gemm_tn_grouped) unless a data-parallel reducer asked for per-layer milestones; the general
    # configurations keep one launch per layer (a grouped launch is another kernel: other numerics)
    grouped = _GROUP_WGRAD and _MILESTONE is None and default and panel

    def dgrad(dy, wt, bits, h, w, b, frag, **rank1):
        """dZ = (dy Wt^T [+ the rank-1 term]) * relu'(H) and the bias gradient of H's layer -> (dZ, db, rows): db is None when it went
        into b.grad or waits in ``rows``, the per-workgroup partial column sums that the layer's weight gradient adds up in its
        reduce launch (weight AND bias accumulate directly: ``_FOLD_BIAS``)."""
        if bits is None:
            dz, ws = ops.gemm_nt(dy, wt, epi=ops.EPI_RANK1_MASK if rank1 else ops.EPI_MASK, mask=h, colsum=True, **rank1)
            return dz, _bgrad(ws, b), None
        fold = _FOLD_BIAS and _direct(w) and _direct(b)
        into = None
        if not fold and _direct(b):                                   # the bias gradient straight from the epilogue
            _touch(b)
            into = b.grad.view(-1)
        dz, _, cs = ops.panel_gemm(dy, wt, ops.PG_RANK1_MASK if rank1 else ops.PG_MASK, bitmask=bits, colsum=True, colsum_into=into,
                                   colsum_defer=fold, frag=frag, **rank1)
        return (dz, None, cs) if fold else (dz, cs, None)

    # decoder (bag level, f32)
    dpre = ops.relu_bwd(dout.contiguous(), out)
    dwd, dbd = _wbgrad(dpre, M, pwd, pbd)
    dM = ops.gemm_nt(dpre, ops.transposed(wd))
    # attention pooling.  From here to the last input gradient a data-parallel step has the head group's all-reduce in flight:
    # these launches leave its channel workgroups their CUs (_overlap_budget: a no-op on one GPU; the default configuration only)
    with _overlap_budget() if default else contextlib.nullcontext():
        direct_k2 = _direct(pba) and _direct(pwb) and _direct(pbb)      # the kernel's atomics add straight into the grads
        if pool_fast:
            # The row scale of the rank-1 term below is A = softmax(s)/sqrt(N), which the forward pass did not form: the bf16 panel
            # kernel makes it from the raw scores and (m, l) in its epilogue; the f32 GEMM takes the rows this pass leaves behind
            dT, dba, dwb, dbb, *att = ops.abmil_pool_bwd(h3.view(B, N, L), wac, ba, wb, scores, ml, M, dM, want_A=not panel, frag=wfrag,
                                                          into=(ba.grad, wb.grad.view(-1), bb.grad) if direct_k2 else None)
            A = att[0] if att else None
        else:
            # any L / D: the generic pooling chain backwards (the forward pass saved U and the soft-max rows as scores, ml; and A)
            dA = ops.rows_dot(h3.view(B, N, L), dM.view(B, 1, L)).view(B, N)
            dAs = ops.mul(dA, torch.full_like(dA, 1.0 / (N ** 0.5)))                               # A = softmax / sqrt(N)
            ds = ops.softmax_rows_bwd(ml, dAs).view(-1)
            dT, dwb, dbb, dba = ops.gated_score_bwd(scores, wb.reshape(-1).contiguous(), ds, gated=False)
            dba = dba.contiguous()
        dwa = _wgrad(dT, h3, pwa)
        if direct_k2:
            _touch(ba, wb, bb)
            _final(wa, ba, wb, bb, wd, bd)
        # encoder layer 3: dZ3 = (dT Wa + A (x) dM) * relu'(H3)
        row_scale = dict(rowscale=scores.view(-1), bias=ml) if panel else dict(rowscale=A.view(-1))
        dz3, db3, rows3 = dgrad(dT, wat, m3, h3, pw3, pb3, False, rank1=dM, rows_per_bag=N, **row_scale)
        if not grouped:
            dw3 = _wgrad(dz3, h2, pw3, pb3, rows3)
            _final(pw3, pb3)
        dz2, db2, rows2 = dgrad(dz3, w3t, m2, h2, pw2, pb2, wfrag)
        if not grouped:
            dw2 = _wgrad(dz2, h1, pw2, pb2, rows2)
            _final(pw2, pb2)
        dz1, db1, rows1 = dgrad(dz2, w2t, m1, h1, pw1, pb1, wfrag)
    # behind the collective: full chip
    if grouped:
        dw3, dw2, dw1 = _wgrad_group([(dz3, h2, w3, b3, rows3), (dz2, h1, w2, b2, rows2), (dz1, x2, w1, b1, rows1)])
        _final(w3, b3, w2, b2, w1, b1)
    else:
        dw1 = _wgrad(dz1, x2, pw1, pb1, rows1)
    dx = ops.gemm_nt(dz1, ops.transpose_cast(w1, T)).view(B, N, d) if need_dx else None
    if direct_k2:
        dba = dwb = dbb = None
    else:
        dba, dwb, dbb = _pgrad(dba, pba), _pgrad(dwb.reshape(1, -1), pwb), _pgrad(dbb, pbb)
    if drop_scale is not None:
        # dZ2 = (dZ3 W3) * relu'(H2) * keep2 and dZ1 = (dZ2 W2) * relu'(H1) * keep1, the masks above hold relu' AND kept
        s2 = drop_scale[1]
        s1 = drop_scale[0] * s2
        dw2, db2, dw1, db1 = dw2 * s2, db2 * s2, dw1 * s1, db1 * s1
        dx = dx * s1 if dx is not None else None
    return dx, dw1, db1, dw2, db2, dw3, db3, dwa, dba, dwb, dbb, dwd, dbd


class ABMILFn(torch.autograd.Function):
    """Whole ABMIL.bag_forward for a batch of equal-length bags (models/abmil.py:35-45).

    x [B,N,d] in the compute dtype (f32 parity path / bf16 throughput path); parameters f32.
    Patch-level tensors (H1..H3, dZ*, dT) live in the compute dtype with f32 accumulation;
    bag-level tensors are f32.  Returns (out [B,L], att, stats): ``attention_rows(att, stats)`` is A [B,N] (non-differentiable).
    """

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, wa, ba, wb, bb, wd, bd, drops=None, grad_on=True):
        """``drops`` = None or the two Dropout(p) keep masks after encoder layers 1 and 2 (abmil.py:12-19): ``ops.DropSeed``s
        (training: the masks are generated inside the passes that apply them) or materialised keep-multiplier tensors
        (values 0 or 1/keep, parity tests).  ``grad_on``: the caller's ``torch.is_grad_enabled()`` - inside ``forward`` autograd
        is always off and ``ctx.needs_input_grad`` stays True for parameters under ``torch.no_grad()``, so only the caller knows
        that no backward pass can follow (frozen encoder of stage 2, validation): then no ReLU masks are written."""
        B, N, d = x.shape
        T = x.dtype
        x2 = x.reshape(B * N, d)
        L = w3.shape[0]
        pool_fast = (L == 512 and wa.shape[0] == 128)       # the one-pass K2 kernel is built for L = 512, D = 128
        wmats = (w1, w2, w3, wa)
        # bf16 + panel-friendly shapes: weight-stationary GEMMs that also emit 1-bit ReLU masks
        fast = abmil_fast_path(B * N, N, d, L, wa.shape[0], T)
        # compute-dtype copies of W1..W3, Wa for this pass and W2^T, W3^T, Wa^T for the dgrads of the backward pass: one launch,
        # and only when a parameter changed since they were last built (ops.weight_views; the fast chain asks for its own)
        tr = [(wa, True, T), (w3, True, T), (w2, True, T)]
        views = None
        if not all(w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() for w in wmats):
            views = [ops.cast(w.contiguous(), T) for w in wmats] + [ops.transpose_cast(w, T) for w in (wa, w3, w2)]
        elif T == torch.float32:
            views = list(wmats) + list(ops.weight_views(tr))
        elif not fast:
            views = ops.weight_views([(w, False, T) for w in wmats] + tr)
        A = None
        if fast:
            keep = bool(grad_on) and any(ctx.needs_input_grad)     # forward-only passes: no ReLU masks to write
            h1, h2, h3, m1, m2, m3, scores, M, ml, out, views = _abmil_fast_forward(
                x2, B, N, (w1, b1, w2, b2, w3, b3, wa, ba, wb, bb, wd, bd), views=views, bits=keep, drops=drops)
        else:
            w1c, w2c, w3c, wac = views[:4]
            m1 = m2 = m3 = None
            h1 = ops.gemm_nt(x2, w1c, epi=ops.EPI_BIAS_RELU, bias=b1)
            if drops is not None:
                _dropout(h1, drops[0], False)
            h2 = ops.gemm_nt(h1, w2c, epi=ops.EPI_BIAS_RELU, bias=b2)
            if drops is not None:
                _dropout(h2, drops[1], False)
            h3 = ops.gemm_nt(h2, w3c, epi=ops.EPI_BIAS_RELU, bias=b3)
            if pool_fast:
                scores, part = ops.abmil_pool_partials(h3.view(B, N, L), wac, ba, wb, bb)
                out, M, ml = ops.abmil_pool_decoder(part, B, N, T, wd, bd)
            else:
                # any L / D (abmil.py:8-30 takes them as arguments): the same attention pooling as a chain of the generic kernels -
                # projection GEMM, tanh score, row soft-max, /sqrt(N) (abmil.py:40-41), weighted row sum
                U = ops.gemm_nt(h3, wac, epi=ops.EPI_BIAS, bias=ba)                                     # [B*N, D]
                s = ops.gated_score_fwd(U, wb.reshape(-1).contiguous(), bb, gated=False).view(B, N)
                Asm = ops.softmax_rows(s)
                A = ops.mul(Asm, torch.full_like(Asm, 1.0 / (N ** 0.5)), out=torch.empty_like(Asm))
                M = ops.weighted_rowsum(h3.view(B, N, L), A.view(B, N, 1)).view(B, L)
                scores, ml = U, Asm                                                                    # what the generic backward needs
                out = ops.gemm_nt(M, wd, epi=ops.EPI_BIAS_RELU, bias=bd)
        wac, wat, w3t, w2t = views[3:]
        ctx.save_for_backward(x2, h1, h2, h3, scores, A, M, ml, out, w1, w2, w3, wa, ba, wb, wd, wac, m1, m2, m3,
                              b1, b2, b3, bb, bd, wat, w3t, w2t)
        ctx.dims = (B, N, d)
        ctx.pool_fast = pool_fast
        # the layout of the K = 512 weight views (wac, w3t, w2t) travels on ctx: ``ops.is_frag`` reads a Python attribute of the
        # tensor object, which a saved-tensor hook that copies (save_on_cpu, a clone) does not carry over to what backward unpacks
        ctx.wfrag = ops.is_frag(wac)
        # the surviving entries of a keep mask all equal 1/keep: the masked dgrads below run unscaled and the (linear) factors
        # are applied to the few gradients behind them
        ctx.drop_scale = None
        if drops is not None:
            ctx.drop_scale = tuple(1.0 / k.keep_q if isinstance(k, ops.DropSeed) else float(k.max().item()) for k in drops)
        # second / third result: what ``attention_rows`` turns into A [B,N] - (raw scores, (m, l)) from the one-pass pooling kernel,
        # (A, None) from the generic chain
        att, stats = (scores, ml) if pool_fast else (A, None)
        ctx.mark_non_differentiable(*([att, stats] if pool_fast else [att]))
        ctx.set_materialize_grads(False)         # no zero-filled dA (a launch) for the attention output nobody differentiates
        return out, att, stats

    @staticmethod
    def backward(ctx, dout, _datt, _dstats):
        _enter(ctx)
        if dout is None:
            return (None,) * 15
        return _abmil_backward(ctx.saved_tensors, ctx.dims, dout, ctx.needs_input_grad[0], ctx.wfrag, pool_fast=ctx.pool_fast,
                               drop_scale=ctx.drop_scale) + (None, None)


def attention_rows(att, stats):
    """The attention rows A [B,N] = softmax(s)/sqrt(N) of an ``ABMILFn`` / ``ABMILStepFn`` call from its second and third result:
    the one-pass pooling kernel hands back raw scores + (m, l) and A costs one small launch HERE, when somebody asks for it
    (``ABMIL.last_attention``); the generic chain already has A."""
    return att if stats is None else ops.abmil_attention(att, stats)


def abmil_fast_path(rows, N, d, L, D, dtype):
    """Does an ABMIL call of this shape take the bf16 weight-stationary encoder + one-pass pooling kernels?"""
    return (dtype == torch.bfloat16 and d == 512 and L == 512 and D == 128 and ops.panel_supported(rows, L, 512, ops.PG_BIAS_RELU)
            and ops.panel_supported(rows, L, 128, ops.PG_RANK1_MASK, N))


DSMILRoute = collections.namedtuple("DSMILRoute", "reassoc qv stream")


@functools.lru_cache(maxsize=None)
def dsmil_route(B, N, d, C, dropped):
    """Which chain a DSMIL call of this shape takes (``DSMILFn`` describes them); ``dropped``: the value branch's input has its own dropout."""
    reassoc, qv = C <= 4, C <= 4 and d % 4 == 0 and d <= 2048
    stream = reassoc and not dropped and ops.dsmil_stream_ok(B, N, d, C)
    assert qv or not stream                  # (the stream plan's d, a multiple of 8 up to 1024, is within dsmil_qv's)
    return DSMILRoute(reassoc, qv, stream)


CLAMRoute = collections.namedtuple("CLAMRoute", "fc_panel fc_bits drop gate dz1_panel inst_fused")


def clam_route(B, N, d, L, D, dtype, gated, keeps, grad_on, needs_grad, inst=None):
    """Which form every stage of a CLAM call takes (``CLAMFn`` describes them).  ``keeps``: None, "seeds" or "tensors"; ``grad_on``: the
    caller's grad mode, ``needs_grad``: some input requires a gradient (both: a backward may follow); ``inst``: None or (n_cls, k_sample, is the
    loss the caller's own).  Not memoised: the parity tests flip the module switches between two calls of one shape; cheap terms come first."""
    rows, bf16, GW, backward = B * N, dtype == torch.bfloat16, (2 * D if gated else D), bool(grad_on and needs_grad)
    fc_panel = bf16 and d == 512 and ops.panel_supported(rows, L, 512, ops.PG_BIAS_RELU)
    drop = None if keeps is None else "injected" if keeps == "tensors" else "epilogue" if (fc_panel and _FUSED_FC_DROP) else \
        "bitmask" if (rows % 32 == 0 and L % 128 == 0) else "mask"
    fc_bits = fc_panel and (drop == "epilogue" or (keeps is None and grad_on))      # that epilogue leaves the 1-bit ReLU mask
    panel = bf16 and L == 512 and ops.panel_supported(rows, GW, 512, ops.PG_BIAS)
    epilogue = panel and gated and GW == 512                # the shapes whose score can come out of the gate GEMM's epilogue
    if _FUSED_GATE and epilogue and keeps is None and not backward and ops.panel_supported(rows, GW, 512, ops.PG_GATE):
        gate = "fused"
    elif (_GATE_U and epilogue and keeps != "tensors" and ops.panel_supported(rows, GW, 512, ops.PG_GATE_U)
          and ops.gated_bwd_il_supported(rows, D, L, N) and ops.panel_supported(rows, L, 512, ops.PG_RANK1_MASK, N)):
        gate = "u"
    else:
        gate = "panel" if panel else "tile"
    dz1_panel = gate == "u" or (backward and bf16 and GW == 512 and ops.panel_supported(rows, L, 512, ops.PG_RANK1_MASK, N))
    inst_fused = inst is not None and not inst[2] and _FUSED_INST and 2 * inst[0] <= 16 and inst[1] <= 32 and L % 8 == 0
    assert D % 16 == 0 or gate in ("panel", "tile")         # (the epilogue gates read the interleaved weight views of ``ops.clam_views``)
    assert dz1_panel or gate != "u"                         # (its backward may group the weight gradients: column sums deferred by the panel dz1 product)
    return CLAMRoute(fc_panel, fc_bits, drop, gate, dz1_panel, inst_fused)


class EncoderSession:
    """ONE aggregator backward for the T patch steps of a sequential training step (train_MuRCL.py:233-304 at train_stage 3).

    The PPO sampler picks step t+1's windows from step t's aggregator states, so the T forward passes cannot be batched -
    but their backward passes can: every step's sub-bags and activations are written into row blocks of ONE set of buffers
    (``x``, ``h1..h3``, ReLU bit masks, scores, pooled vectors), the per-step autograd nodes (``ABMILStepFn``) only collect their
    upstream gradients, and the node autograd reaches last runs the backward kernels once over all T * bags bags: each dgrad /
    wgrad / pooling-backward kernel once at full size instead of T times at 1/T of it (a launch costs ~15 us before its first tile
    and the weight gradients re-reduce their partial tiles per launch)."""

    def __init__(self, steps, bags, N, d, L, dtype, device):
        self.steps, self.bags, self.N, self.d, self.L = steps, bags, N, d, L
        R, Bt = steps * bags * N, steps * bags
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)      # noqa: E731
        self.x = e((steps, bags, N, d), dtype)
        self.h1, self.h2, self.h3 = e((R, L), dtype), e((R, L), dtype), e((R, L), dtype)
        self.m1, self.m2, self.m3 = (e((R, L // 8), torch.uint8) for _ in range(3))
        self.scores = e((Bt, N), torch.float32)
        self.M, self.ml, self.out = e((Bt, L), torch.float32), e((Bt, 2), torch.float32), e((Bt, L), torch.float32)
        self.t, self.pending, self.dout, self.weights = 0, 0, [None] * steps, None

    def views(self, t):
        """The [bags, N, d] block step t's sub-bags are gathered into (``subbag_views(out=...)``)."""
        return self.x[t]

    def rows(self, buf, t, per=None):
        per = self.bags * self.N if per is None else per
        return buf[t * per:(t + 1) * per]


class ABMILStepFn(torch.autograd.Function):
    """One patch step's ABMIL forward inside an ``EncoderSession`` (default shape, bf16): same kernels as ``ABMILFn``, results in
    the session's row blocks; the backward only files its upstream gradient until the session's last node runs them all."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, wa, ba, wb, bb, wd, bd, session):
        s, t = session, session.t
        B, N, d = x.shape
        if not (t < s.steps and (B, N, d) == (s.bags, s.N, s.d)):
            # (a session left behind by a step that raised: drop it rather than trip every later call)
            raise RuntimeError("EncoderSession: shape / step count differ from what it was built for - a previous step may have "
                               "raised before clearing model.encoder.session; set it to None")
        x2 = s.x[t].view(B * N, d)
        if x.data_ptr() != x2.data_ptr():
            x2.copy_(x.reshape(B * N, d))
        blk = lambda buf: s.rows(buf, t, B)                                          # noqa: E731
        blocks = (s.rows(s.h1, t), s.rows(s.h2, t), s.rows(s.h3, t), s.rows(s.m1, t), s.rows(s.m2, t), s.rows(s.m3, t),
                  blk(s.scores), (blk(s.out), blk(s.M), blk(s.ml)))
        _h1, _h2, _h3, _m1, _m2, _m3, scores, _M, ml, out, views = _abmil_fast_forward(
            x2, B, N, (w1, b1, w2, b2, w3, b3, wa, ba, wb, bb, wd, bd), blocks=blocks)
        wac, wat, w3t, w2t = views[3:]
        s.weights = (w1, w2, w3, wa, ba, wb, wd, wac, b1, b2, b3, bb, bd, wat, w3t, w2t)
        s.wfrag = ops.is_frag(wac)
        s.t, s.pending = t + 1, s.pending + 1
        ctx.session, ctx.t = s, t
        ctx.mark_non_differentiable(scores, ml)
        ctx.set_materialize_grads(False)
        return out, scores, ml

    @staticmethod
    def backward(ctx, dout, _datt, _dstats):
        s = ctx.session
        s.dout[ctx.t] = dout
        s.pending -= 1
        if s.pending > 0:
            return (None,) * 14
        n = s.t                                                                      # steps that ran
        if all(g is None for g in s.dout[:n]):
            return (None,) * 14
        like = next(g for g in s.dout[:n] if g is not None)
        _enter(ctx)                                                                  # (every step's node has the same parameter inputs)
        from .utils.views import adjacent as _adjacent, as_one as _as_one       # (module level would be a circular import)
        douts = [g if g is not None else torch.zeros_like(like) for g in s.dout[:n]]
        if all(g is not None for g in s.dout[:n]) and _adjacent(douts):
            dout_all = _as_one(douts)                                                # row blocks of one gradient (SessionOutFn): a re-view
        else:
            dout_all = torch.cat([g.contiguous() for g in douts], 0)
        (w1, w2, w3, wa, ba, wb, wd, wac, b1, b2, b3, bb, bd, wat, w3t, w2t) = s.weights
        R, Bt = n * s.bags * s.N, n * s.bags
        saved = (s.x.view(-1, s.d)[:R], s.h1[:R], s.h2[:R], s.h3[:R], s.scores[:Bt], None, s.M[:Bt], s.ml[:Bt], s.out[:Bt],
                 w1, w2, w3, wa, ba, wb, wd, wac, s.m1[:R], s.m2[:R], s.m3[:R], b1, b2, b3, bb, bd, wat, w3t, w2t)
        return _abmil_backward(saved, (Bt, s.N, s.d), dout_all, False, s.wfrag, pool_fast=True, drop_scale=None) + (None,)


class SessionOutFn(torch.autograd.Function):
    """The aggregator outputs of all patch steps of an ``EncoderSession`` as ONE tensor [steps * bags, L] without a copy: the steps
    wrote them into consecutive row blocks of ``session.out``, so the forward is a view of that buffer and the backward hands every
    step the row block of the ONE upstream gradient that belongs to it (views again: ``ABMILStepFn.backward`` then finds its T
    upstream gradients adjacent in one buffer).  Replaces a concatenation of 2T tensors in the forward pass and, in the backward pass,
    T concatenations of the two views' gradients plus one of the T steps' (stage 3 of train_MuRCL.py: 8 ATen launches)."""

    @staticmethod
    def forward(ctx, session, *hs):
        ctx.n, ctx.rows = len(hs), session.bags
        ctx.set_materialize_grads(False)
        return session.out[:len(hs) * session.bags].view(len(hs) * session.bags, -1)

    @staticmethod
    def backward(ctx, d):
        if d is None:
            return (None,) * (1 + ctx.n)
        d = d.contiguous()
        return (None,) + tuple(d[t * ctx.rows:(t + 1) * ctx.rows] for t in range(ctx.n))


def session_whole(session, hs):
    """``hs`` = the per-step aggregator outputs [bags, L] of ``session`` in step order -> the [steps * bags, L] tensor that equals
    ``torch.cat(hs)`` (a view of the session's buffer, differentiable), or None when they are not the session's row blocks."""
    if session is None or not hs or len(hs) > session.steps:
        return None
    row = session.out.shape[1] * session.out.element_size()
    for t, h in enumerate(hs):
        if not (torch.is_tensor(h) and h.dtype == session.out.dtype and tuple(h.shape) == (session.bags, session.out.shape[1])
                and h.is_contiguous() and h.data_ptr() == session.out.data_ptr() + t * session.bags * row):
            return None
    return SessionOutFn.apply(session, *hs)


def _gru_forward(x2, B, zero_blocks, w_ih, w_hh, b_ih, b_hh, *, h_prev=None, step=False, keep=True):
    """nn.GRU (PyTorch gate order) over x2 [n*B, I] f32 = n blocks of B rows: the first ``zero_blocks`` blocks start from the zero state,
    block k >= ``zero_blocks`` continues from block k-1 - or, a single block with ``zero_blocks`` = 0, from the external ``h_prev`` [B,H].
    The layouts: one step (n = 1), nn.GRU over a rollout (T blocks, 1 from zero), the 2T aggregator outputs of a contrastive step
    x_00, x_01, x_10, x_11, ... (2 from zero: ``restart`` at patch step 0, then the reference's one shared hidden state).
    ``step``: a single cell, whose input product joins the gate launch where the kernel takes it; every other layout forms the input
    projection of all rows as ONE GEMM.  ``keep``: also produce what ``_gru_backward`` reads.
    -> (hs [n*B, H]: every hidden state in one buffer, gates [n*B, 3H], gh [n*B, 3H]); without ``keep`` the last two are None.
    The zero-state rows of gh stay unwritten: W_hh . 0 + b_hh is ONE row, b_hh, that every such row reads."""
    R, H = x2.shape[0], w_hh.shape[1]
    n, z = R // B, zero_blocks
    assert R == n * B and 0 <= z <= n and (h_prev is None) == (z > 0) and (h_prev is None or n == 1) and (not step or n == 1)
    wih, whh, bih, bhh = w_ih.detach(), w_hh.detach(), b_ih.detach(), b_hh.detach()
    if step and x2.dtype == torch.float32 and ops.gru_step_ok(B, H, x2.shape[1]) and (h_prev is None or not keep):
        # both products of the cell (from the zero state: the input product) and the gate math in one launch; a continuing step
        # that a backward pass may follow has always taken the chain below instead (gemm_nt + the one-launch step)
        hs, gates, _ = ops.gru_step_fwd(bih, h_prev, whh, bhh, x=x2, w_ih=wih, want_backward=keep, want_gh=False)
        return hs, gates, None
    # h W_hh^T and the gate math of a continuing block in one launch, or gemm_nt + gate kernel.  (A forward-only step that the form
    # above refused - an input width that is no multiple of 16 - has always taken the latter.)
    fused = ops.gru_step_ok(B, H) and (keep or not step)
    e = lambda cols, on=True: torch.empty((R, cols), dtype=torch.float32, device=x2.device) if on else None      # noqa: E731
    blk = lambda t, k: None if t is None else t[k * B:(k + 1) * B]                                               # noqa: E731
    gi = ops.gemm_nt(x2, wih, epi=ops.EPI_BIAS, bias=bih)
    hs, gates, gh = e(H), e(3 * H, keep), e(3 * H, n > z and (keep or not fused))
    if z:
        ops.gru_gates_fwd(gi[:z * B], bhh.view(1, -1), None, hnew=hs[:z * B], gates=None if gates is None else gates[:z * B])
    for k in range(z, n):
        prev = blk(hs, k - 1) if k else h_prev
        if fused:
            ops.gru_step_fwd(blk(gi, k), prev, whh, bhh, hnew=blk(hs, k), gates=blk(gates, k), gh=blk(gh, k) if keep else None,
                             want_backward=keep)
        else:
            ops.gemm_nt(prev, whh, epi=ops.EPI_BIAS, bias=bhh, out=blk(gh, k))
            ops.gru_gates_fwd(blk(gi, k), blk(gh, k), prev, hnew=blk(hs, k), gates=blk(gates, k))
    return hs, gates, (gh if keep else None)


def _gru_backward(gates, gh, hs, h_prev, gh0, B, zero_blocks, dhs, w_hh_t):
    """Back through the blocks of ``_gru_forward`` (what it kept; ``gh0`` = b_hh as one row; ``dhs`` [n*B, H] contiguous; ``w_hh_t`` =
    W_hh^T, not read for a single block) -> (dgi, dgh [n*B, 3H], dhp): dhp [B,H] = the direct path dh * z into an external ``h_prev``,
    to which the caller adds dgh W_hh; None without one."""
    R, H = dhs.shape
    n, z = R // B, zero_blocks
    blk = lambda t, k: t[k * B:(k + 1) * B]                                              # noqa: E731
    dgi = torch.empty((R, 3 * H), dtype=torch.float32, device=dhs.device)
    dgh = torch.empty_like(dgi)
    if n > max(z, 1) and ops.gru_step_ok(B, H):
        # one launch per block: dh_{k-1} += dgh_k W_hh, then block k-1's gate backward on the finished rows; the working copy of the
        # upstream gradients also collects the direct path dh_k * z_k of every block
        work = ops.copy_flat(torch.empty_like(dhs), dhs)
        ops.gru_gates_bwd_into(blk(work, n - 1), blk(gates, n - 1), blk(gh, n - 1), blk(hs, n - 2), blk(dgi, n - 1), blk(dgh, n - 1),
                               blk(work, n - 2), accumulate=True)
        for k in range(n - 1, z - 1, -1):
            zero = k - 1 < z                  # block k-1 started from the zero state: the bias row, no previous state to pass a gradient to
            ops.gru_step_bwd(blk(dgh, k), w_hh_t, blk(work, k - 1), blk(gates, k - 1), gh0 if zero else blk(gh, k - 1),
                             None if zero else blk(hs, k - 2), blk(dgi, k - 1), blk(dgh, k - 1), None if zero else blk(work, k - 2),
                             accumulate=True)
        if z > 1:                             # the zero-state blocks nothing continued from: single steps beside the chain
            rows = slice(0, (z - 1) * B)
            ops.gru_gates_bwd_into(work[rows], gates[rows], gh0, None, dgi[rows], dgh[rows])
        return dgi, dgh, None
    carry = dhp = None
    for k in range(n - 1, -1, -1):
        cont = k >= z
        dh = blk(dhs, k) if carry is None else blk(dhs, k) + carry
        _, _, dhp = ops.gru_gates_bwd(dh, blk(gates, k), blk(gh, k) if cont else gh0, (blk(hs, k - 1) if k else h_prev) if cont else None,
                                      dgi=blk(dgi, k), dgh=blk(dgh, k))
        carry = ops.gemm_nt(blk(dgh, k), w_hh_t, out=dhp, accumulate=True) if cont and k else None
    return dgi, dgh, (dhp if h_prev is not None else None)


def _gru_param_grads(dgi, dgh, x2, hs, h_prev, B, zero_blocks, w_ih, w_hh, b_ih, b_hh, split_bias):
    """-> (dw_ih, dw_hh, db_ih, db_hh) of a ``_gru_forward`` pass.  ``split_bias``: the input side as ``_wgrad`` + ``_bgrad`` (two
    launches, never deferred - what the rollout layout has always run) instead of ``_wbgrad``."""
    R, z = x2.shape[0], zero_blocks
    db_ih = db_hh = None
    if split_bias:
        dw_ih = _wgrad(dgi, x2, w_ih)
    else:
        dw_ih, db_ih = _wbgrad(dgi, x2, w_ih, b_ih)
    if h_prev is not None:
        dw_hh, db_hh = _wbgrad(dgh, h_prev, w_hh, b_hh)
    elif R > z * B:
        dw_hh = _wgrad(dgh[z * B:], hs[(z - 1) * B:R - B], w_hh)          # blocks k >= z against the state of block k-1
    else:
        # nn.GRU from a zero state: a zero gradient, but a gradient (Adam applies decay) - announced here when direct, by
        # AccumulateGrad's hook otherwise (and not at all when this backward pass does not accumulate into w_hh)
        dw_hh = _touch(w_hh) if _direct(w_hh) else torch.zeros_like(w_hh)        # (_touch returns None)
    if split_bias:
        db_ih = _bgrad(dgi, b_ih)
    if h_prev is None:
        db_hh = _bgrad(dgh, b_hh)
    return dw_ih, dw_hh, db_ih, db_hh


class GRUFn(torch.autograd.Function):
    """``_gru_forward`` over the row blocks of x [n*B, I] (or [n, B, I]) as ONE node -> every hidden state, in x's leading shape.  The
    input projection, the input gradient and each weight / bias gradient are ONE launch over all n*B rows; only h W_hh^T and the gate
    kernels stay inside the loop over blocks."""

    @staticmethod
    def forward(ctx, x, h_prev, w_ih, w_hh, b_ih, b_hh, B, zero_blocks, step, split_bias):
        x2 = _flat2(x).contiguous()
        h_prev = None if h_prev is None else h_prev.contiguous()
        hs, gates, gh = _gru_forward(x2, B, zero_blocks, w_ih, w_hh, b_ih, b_hh, h_prev=h_prev, step=step)
        ctx.save_for_backward(x2, h_prev, w_ih, w_hh, gates, gh, hs, b_ih, b_hh)
        ctx.layout = (B, zero_blocks, step, split_bias, x.shape)
        return hs if x.dim() == 2 else hs.view(*x.shape[:-1], hs.shape[1])

    @staticmethod
    def backward(ctx, dhs):
        _enter(ctx)
        x2, h_prev, w_ih, w_hh, gates, gh, hs, b_ih, b_hh = ctx.saved_tensors
        B, z, step, split_bias, xshape = ctx.layout
        # (every layout but the single step forms W_hh^T up front - a rollout of one block too, which does not read it)
        w_hh_t = None if step else ops.transposed(w_hh)
        dgi, dgh, dhp = _gru_backward(gates, gh, hs, h_prev, b_hh.detach().view(1, -1), B, z, _flat2(dhs).contiguous(), w_hh_t)
        dx = ops.gemm_nt(dgi, ops.transposed(w_ih)).view(xshape) if ctx.needs_input_grad[0] else None
        grads = _gru_param_grads(dgi, dgh, x2, hs, h_prev, B, z, w_ih, w_hh, b_ih, b_hh, split_bias)
        dh_prev = None
        if h_prev is not None and ctx.needs_input_grad[1]:
            dh_prev = ops.gemm_nt(dgh, ops.transposed(w_hh), out=dhp, accumulate=True)
        return (dx, dh_prev) + grads + (None,) * 4


class GRUStepFn:
    """One nn.GRU time step (seq_len 1); ``h_prev`` None == zeros."""

    @staticmethod
    def apply(x, h_prev, w_ih, w_hh, b_ih, b_hh):
        return GRUFn.apply(x, h_prev, w_ih, w_hh, b_ih, b_hh, x.shape[0], int(h_prev is None), True, False)


class GRUSeqFn:
    """nn.GRU over a whole rollout from a zero hidden state (ActorCritic.evaluate, models/rlmil.py:99-112): x [T,B,I] -> all hidden
    states [T,B,H]."""

    @staticmethod
    def apply(x, w_ih, w_hh, b_ih, b_hh):
        return GRUFn.apply(x, None, w_ih, w_hh, b_ih, b_hh, x.shape[1], 1, False, True)


class NTXentSeqFn(torch.autograd.Function):
    """NT_Xent of T independent (view 0, view 1) batches at once: z [T,2B,P] -> (loss [T], cos(z_i, z_j) [T,B]); one launch
    computes all losses, gradients and cosines (the T patch steps of a pre-training step, train_MuRCL.py:249,277)."""

    @staticmethod
    def forward(ctx, z, temperature):
        """-> (loss [T], sim [T,B], mean of the T losses): the step loss of train_MuRCL.py:291 comes out of this node as its own
        launch (``ops.mean_small``), so that its gradient - 1/T on every step - is ONE scaling of the stored dz instead of a mean
        node's reduce, expand and multiply."""
        loss, dz, sim = ops.ntxent_batched(z, temperature, want_grad=True)
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(sim)
        ctx.set_materialize_grads(False)
        return loss, sim, ops.mean_small(loss)

    @staticmethod
    def backward(ctx, dloss, _dsim, dmean):
        (dz,) = ctx.saved_tensors
        if dloss is None and dmean is None:
            return None, None
        T_ = dz.shape[0]
        if dloss is None and ops.is_unit_grad(dmean):
            return ops.axpby(dz, dz, 1.0 / T_, 0.0), None                                # (b = 0: y is not read)
        w = dloss if dmean is None else (dmean / T_).expand(T_) if dloss is None else dloss + dmean / T_
        return dz * w.reshape(-1, 1, 1), None


class NTXentFn(torch.autograd.Function):
    """NT_Xent.forward (utils/losses.py:24-41); gradient comes out of the same launch."""

    @staticmethod
    def forward(ctx, z_i, z_j, temperature, grad_lo, grad_hi):
        # z_j None: z_i already is the stacked [2B,P] batch (both views came out of one GEMM: no concatenation)
        z = z_i if z_j is None else torch.cat([z_i, z_j], 0)
        loss, dz, sim = ops.ntxent(z, temperature, want_grad=True, grad_lo=grad_lo, grad_hi=grad_hi)
        ctx.save_for_backward(dz)
        ctx.B = z.shape[0] // 2
        ctx.joint = z_j is None
        ctx.mark_non_differentiable(sim)
        ctx.set_materialize_grads(False)
        return loss[0], sim

    @staticmethod
    def backward(ctx, dloss, _dsim):
        (dz,) = ctx.saved_tensors
        if dloss is None:
            return None, None, None, None, None
        g = dz if ops.is_unit_grad(dloss) else dz * dloss
        if ctx.joint:
            return g, None, None, None, None
        return g[:ctx.B], g[ctx.B:], None, None, None


class DSMILFn(torch.autograd.Function):
    """MILNet.forward for a batch of equal-length bags (models/dsmil.py:9-16,64-81,104-113).

    The value projection is applied AFTER pooling: bag = (A^T X) Wv^T + bv, identical to A^T (X Wv^T + bv) because every column
    of the soft-max sums to one.  The query projection is reassociated the same way (round 3): the attention logits
    Q[n] . q_c / sqrt(128) with Q = X Wq^T + bq equal X[n] . v_c + const for v_c = Wq^T q_c / sqrt(128), and the soft-max over n
    ignores the constant - the [B*N, 128] queries and the two GEMMs over all patches (forward and dWq) are never formed.

    ``dsmil_route`` picks the chain once, in ``forward``; ``backward`` reads the stored route:
      stream   (no dropout_v, and ``ops.dsmil_stream_ok`` covers the shape - among its terms C <= 2, d <= 1024): instance scores, attention + pooling
               (``ops.dsmil_attn_pool``) and their whole backward with dWc (``ops.dsmil_attn_pool_bwd``) are one pass over X each, around
               three launches of [B*C]-row algebra (``ops.dsmil_qv``, ``ops.dsmil_qv_bwd``);
      explicit (any other C <= 4): the same algebra as separate passes (rows_dot, soft-max, weighted_rowsum and their backward);
               ``route.qv`` (d % 4 == 0, d <= 2048) keeps ``ops.dsmil_qv`` in front of them;
      literal  (C > 4): the reference's order - queries by one GEMM over all patches, a 3-term bf16 split in f32; the row kernels
               keep four classes in registers, so ops.py launches them once per group of four classes.
    Returns (classes [B,N,C], bag [B,C,d], m [B,C], cmax [B,C]).
    """
    QD = 128

    @staticmethod
    def forward(ctx, x, wc, bc, wq, bq, wv, bv, want_max=False, keep_v=None):
        """``keep_v`` (BClassifier(dropout_v > 0) in training mode, dsmil.py:53-59: ``v = Linear(Dropout(feats))``): None, or a keep
        multiplier for the VALUE branch's input - an ``ops.DropSeed`` (its mask is materialised here: a path no script takes) or a
        [B,N,d] tensor of 0 / 1/keep (parity tests).  The attention logits see the un-dropped features (``q = Linear(feats)``), so the
        pooled operand is X * keep while scores and logits use X: the explicit chain (soft-max, then a weighted row sum over the
        dropped copy) instead of the one-pass kernels.
        ``want_max``: also return cmax [B,C] = the max-instance class scores (train_RLMIL.py:516, ``torch.max(outputs_ins, 0)``) as a
        differentiable output - the arg-max launch has them in hand, and their gradient reaches the instance classifier through the
        B*C critical rows only (no dense [B,N,C] gradient, no ATen max / scatter / fill launches)."""
        B, N, d = x.shape
        T, C, QD = x.dtype, wc.shape[0], DSMILFn.QD
        assert wq.shape[0] == QD
        route = dsmil_route(B, N, d, C, keep_v is not None)
        scale = 1.0 / math.sqrt(QD)
        x2 = x.reshape(B * N, d)
        xv = x                                                                          # the value branch's input (dsmil.py:66)
        if keep_v is not None:
            km = ops.dropout_mask((B, N, d), T, keep_v.keep_p, x.device, seed=keep_v.seed) if isinstance(keep_v, ops.DropSeed) else \
                keep_v.to(T).reshape(B, N, d).contiguous()
            xv = ops.mul(x, km, out=torch.empty_like(x))
        cls = ops.rows_dot(x2.view(1, B * N, d), wc.view(1, C, d), bias=bc).view(B * N, C)    # instance scores (dsmil.py:9-16)
        m, cmax = ops.dsmil_argmax(cls, B, N, C, want_max=True)                         # critical instances (:71-73) and their scores
        # front: the critical instances' queries q_c and - reassociated - v_c = Wq^T q_c; literal: the queries Q of all patches
        xm = Q = None
        if route.qv:
            xm, qmax, v = ops.dsmil_qv(x2, m, wq, bq, B, N, C)                          # x_m, q_c = Wq x_m + bq, Wq^T q_c: one launch
        elif route.reassoc:
            x_m = ops.cast(ops.gather_rows(x2, m, B, C, N, 0, d), torch.float32)        # [B*C, d]
            qmax = ops.gemm_nt(x_m, wq, epi=ops.EPI_BIAS, bias=bq)                      # q_c = Wq x_m + bq     [B*C, 128]
            v = ops.gemm_nt(qmax, ops.transposed(wq))                                   # Wq^T q_c              [B*C, d]
        else:
            # one 128-column GEMM [B*N, 128]; f32: as a 3-term bf16 split on the bf16 matrix pipe (ops.gemm_nt x3)
            Q = ops.gemm_nt(x2, wq if T == torch.float32 else ops.cast(wq, T), epi=ops.EPI_BIAS, bias=bq, out_dtype=torch.float32, x3=True)
            qmax = ops.gather_rows(Q, m, B, C, N, 0, QD)
        # middle: A = soft-max_n(X v_c / sqrt(128)) (:76-77) and Z = A^T X (:78; X * keep with dropout_v)
        if route.stream:
            one = ops.dsmil_attn_pool(x, v.view(B, C, d), scale)                        # both from one pass over X
            assert one is not None
            A, Z = one
        else:
            A = ops.dsmil_softmax_(ops.rows_dot(x, v.mul_(scale).view(B, C, d))) if route.reassoc else ops.dsmil_attn(Q, 0, qmax, B, N, C)
            Z = ops.weighted_rowsum(xv, A)
        bag = ops.gemm_nt(Z.view(B * C, d), wv, epi=ops.EPI_BIAS, bias=bv).view(B, C, d)    # tail: the value projection of the pooled rows
        none = _placeholder(x)
        ctx.save_for_backward(x, m, qmax, A, Z, wv, wq, Q if Q is not None else none, xm if xm is not None else none,
                              xv if keep_v is not None else none)
        ctx.meta = (B, N, d, C, route, keep_v is not None)
        ctx.params = (wc, bc, wq, bq, wv, bv)             # (the parameters themselves: the backward pass adds into their gradient buffers)
        ctx.mark_non_differentiable(m)
        ctx.set_materialize_grads(False)
        if not want_max:
            ctx.mark_non_differentiable(cmax)
        return cls.view(B, N, C), bag, m, cmax

    @staticmethod
    def backward(ctx, dclasses, dbag, _dm, dcmax=None):
        _enter(ctx)
        x, m, qmax, A, Z, wv, wq, Q, xm, xv = ctx.saved_tensors
        B, N, d, C, route, dropped = ctx.meta
        xv = xv if dropped else x                                                           # the pooled operand (X * keep under dropout_v)
        T, QD, dev = x.dtype, DSMILFn.QD, x.device
        scale = 1.0 / math.sqrt(QD)
        x2 = x.reshape(B * N, d)
        dbag2 = (dbag if dbag is not None else torch.zeros((B, C, d), device=dev)).reshape(B * C, d).contiguous()
        dwv, dbv = ops.gemm_tn_with_colsum(dbag2, Z.view(B * C, d))                         # value side: (dWv, dbv) in one launch, and dZ
        dZ = ops.gemm_nt(dbag2, ops.transposed(wv)).view(B, C, d)
        if not route.qv:
            xm = ops.gather_rows(x2, m, B, C, N, 0, d)                                      # critical instances (dsmil_qv saved its own, in f32)
        dcls = dclasses.reshape(B, N, C).float().contiguous() if dclasses is not None else None
        # attention and pooling -> R = dL/dv_c (literal: dQ, dqmax), and the dense dWc = dcls^T X where the pass over X gives it on the way
        if route.stream:
            one = ops.dsmil_attn_pool_bwd(x, dZ, A, Z, dcls, scale)                         # ONE pass over X: neither dA nor dS is stored
            assert one is not None
            R, dwc = one[0].view(B * C, d), one[1]
        else:
            # dA = (X * keep) dZ^T and, when the instance scores carry a gradient, dWc from the SAME pass over X
            fused = ops.rows_dot_wsum(x, dZ, dcls) if (dcls is not None and not dropped) else None
            dA, dwc = fused if fused is not None else (ops.rows_dot(xv, dZ), None)
            if route.reassoc:
                R = ops.weighted_rowsum(x, ops.dsmil_softmax_bwd(A, dA)).view(B * C, d)     # dS weights the rows of X once more:
                R *= scale                                                                  # R_c = sum_n dS[n,c] X[n] / sqrt(128)
            else:
                dQ = torch.empty((B * N, QD), dtype=torch.float32, device=dev)              # written in full below
                dqmax = ops.dsmil_attn_bwd(A, dA, Q, 0, qmax, dQ, B, N, C)
        if route.stream and dcmax is not None:
            # query side and instance classifier in one: dsmil_qv_bwd's second launch adds the max-instance term of (dWc, dbc) to the dense one
            dwc, dbc = (dwc, dcls.view(B * N, C).sum(0)) if dcls is not None else \
                (torch.empty((C, d), dtype=torch.float32, device=dev), torch.empty((C,), dtype=torch.float32, device=dev))
            dwq, dbq = ops.dsmil_qv_bwd(R, qmax, xm, wq, dcmax=dcmax.float(), dwc=dwc, dbc=dbc, accumulate=dcls is not None)
        else:
            if route.stream:                                                                # query side
                dwq, dbq = ops.dsmil_qv_bwd(R, qmax, xm, wq)                                # dq = R Wq^T, dWq = q^T R + dq^T x_m, dbq
            elif route.reassoc:
                # sum_n dQ[n]^T X[n] = qmax^T R,  dqmax = sum_n dS[n,c] Q[n] / sqrt(128) = R Wq^T (+ bq sum_n dS[n,c]: a soft-max gradient sums to 0)
                dqmax = ops.gemm_nt(R, wq)                                                  # [B*C, 128]
                dwq = ops.gemm_tn(qmax, R)                                                  # [128, d]
                ops.gemm_tn(dqmax, xm if route.qv else ops.cast(xm, torch.float32), out=dwq)
                dbq = ops.colsum(dqmax)
            else:
                dwq = ops.gemm_tn(dQ if T == torch.float32 else ops.cast(dQ, T), x2, x3=True)   # [128, d]: one tile row
                dbq = ops.colsum(dQ)
                ops.gemm_tn(dqmax if T == torch.float32 else ops.cast(dqmax, T), xm, out=dwq)
                ops.colsum(dqmax, out=dbq, accumulate=True)
            # instance classifier, dense term: where no pass over X gave dWc above, a weighted row sum over all patches (not a 128-wide wgrad tile) ...
            dbc = None
            if dcls is not None:
                if dwc is None:
                    dwc = ops.weighted_rowsum(x2.view(1, B * N, d), dcls.view(1, B * N, C)).view(C, d)
                dbc = dcls.view(B * N, C).sum(0)
            if dcmax is not None:
                # ... and the max-instance term: the same sums as dsmil_qv_bwd's, in plain tensor ops on the B*C critical rows
                xm_f = (xm if route.qv else ops.cast(ops.gather_rows(x2, m, B, C, N, 0, d), torch.float32)).view(B, C, d)
                g = dcmax.float().view(B, C, 1)
                dwc_m, dbc_m = (g * xm_f).sum(0), g.view(B, C).sum(0)
                dwc = dwc_m if dwc is None else dwc + dwc_m
                dbc = dbc_m if dbc is None else dbc + dbc_m
        # six parameter gradients: ONE launch adds them to the optimizer's pre-seated buffers (no AccumulateGrad add per parameter)
        dwc, dbc, dwq, dbq, dwv, dbv = _pgrads(*zip((dwc, dbc, dwq, dbq, dwv, dbv), ctx.params))
        return None, dwc, dbc, dwq, dbq, dwv, dbv, None, None


_INST_CONST = {}
_ZERO_CONST = {}


def _zeros_const(dev, n):
    """A shared read-only zero vector (the instance loss of a call without instance evaluation): no fill launch per call."""
    z = _ZERO_CONST.get((dev, n))
    if z is None:
        z = _ZERO_CONST[(dev, n)] = torch.zeros((n,), dtype=torch.float32, device=dev)
    return z


def _placeholder(like):
    """A shared one-element tensor that stands in for an absent saved tensor (``save_for_backward`` takes tensors): no fill launch per call."""
    key = (like.device, like.dtype, "placeholder")
    z = _ZERO_CONST.get(key)
    if z is None:
        z = _ZERO_CONST[key] = torch.zeros((1,), dtype=like.dtype, device=like.device)
    return z


def _inst_constants(dev, B, N, k, n_cls, subtyping):
    """Index / target constants of CLAM's instance branch, built once per shape (they were five tiny launches and three
    host->device copies per call): bag row offsets [B,1], class ids [1,n_cls], in-class targets [1,1,2k] = [1]*k + [0]*k
    (clam.py:105-119), out-of-class targets [0]*k (subtyping, clam.py:122-132) or none, the rest ignored (-1)."""
    key = (dev, B, N, k, n_cls, bool(subtyping))
    c = _INST_CONST.get(key)
    if c is None:
        if len(_INST_CONST) > 32:
            _INST_CONST.clear()
        base = (torch.arange(B, device=dev, dtype=torch.int64) * N).unsqueeze(1)
        cls_ids = torch.arange(n_cls, device=dev).view(1, n_cls)
        t_in = torch.tensor([1] * k + [0] * k, dtype=torch.int64, device=dev).view(1, 1, -1)
        t_out = torch.tensor(([0] * k if subtyping else [-1] * k) + [-1] * k, dtype=torch.int64, device=dev).view(1, 1, -1)
        c = _INST_CONST[key] = (base, cls_ids, t_in, t_out)
    return c


class StackParamsFn(torch.autograd.Function):
    """``torch.stack`` of the n instance classifiers' weights and of their biases (clam.py:103-132 reads them per class) -> ([n,R,L],
    [n,R]) as one launch - none between optimizer steps (``ops.stacked_views``) - instead of two ATen concatenations per forward;
    the backward hands every parameter its slice of the stacked gradient (no launch)."""

    @staticmethod
    def forward(ctx, n, *params):
        ws, bs = params[:n], params[n:]
        W, b = ops.stacked_views(ws, bs)
        ctx.n = n
        return W.view(n, *ws[0].shape), b.view(n, *bs[0].shape)

    @staticmethod
    def backward(ctx, dW, db):
        n = ctx.n
        gw = [None] * n if dW is None else [dW[i] for i in range(n)]
        gb = [None] * n if db is None else [db[i] for i in range(n)]
        return (None, *gw, *gb)


CLAMInstFused = collections.namedtuple("CLAMInstFused", "ids dl w_st k n_cls")                  # what each form of CLAM's instance
CLAMInstExplicit = collections.namedtuple("CLAMInstExplicit", "rows feats dl scale k n_cls")    # branch keeps for its backward


def _clam_first_layer(route, x2, w1c, b1, k1):
    """h = Dropout(ReLU(x W1^T + b1)) (clam.py:69-72) -> (h, m1): m1 = the 1-bit mask of h > 0 for the panel dz1 product, or None."""
    if route.fc_panel:
        # weight-stationary panel kernel; its 1-bit ReLU mask also serves the backward pass.  Seeded Dropout(0.25) behind the ReLU
        # happens in the same epilogue: the mask is never materialised and the bits record what survives
        h, m1, _ = ops.panel_gemm(x2, w1c, ops.PG_BIAS_RELU, bias=b1, want_bitmask=route.fc_bits, drop=k1 if route.drop == "epilogue" else None)
    else:
        h, m1 = ops.gemm_nt(x2, w1c, epi=ops.EPI_BIAS_RELU, bias=b1), None
    if route.drop == "bitmask":
        # the mask is generated inside the pass that applies it, which also leaves the 1-bit mask of the surviving positive entries (bf16 panel dgrad)
        m1 = ops.dropout_relu_bitmask(h, k1, want_bits=h.dtype == torch.bfloat16)
    elif route.drop in ("mask", "injected"):                                       # a materialised mask; a keep mask from the caller (parity tests)
        ops.mul(h, k1 if route.drop == "injected" else ops.dropout_mask(h.shape, h.dtype, k1.keep_p, h.device, seed=k1.seed))
    return h, m1


def _clam_gate(route, h, B, N, gate_params, views, c, ka, kb):
    """Attention scores, soft-max over the bag and pooling (clam.py:18-56,144,170) -> (U or None, s [B,N], A [B,N], M [B,L])."""
    wa, ba, wb, bb, wc, bc = gate_params
    gated, L = wb is not None, h.shape[1]
    if route.gate in ("fused", "u"):
        # fused - forward-only calls (validation, heat-map scoring, the frozen aggregator of stage 2): the score comes out of the gate
        # GEMM's epilogue - tanh(a_d) sigmoid(b_d) c_d summed per wave - and the [B*N, 2D] pre-activations are never written
        # u - calls a backward pass may follow: the same epilogue also leaves the pre-activations (interleaved column order) for it,
        # and the separate score pass over U (97-120 us at C3) disappears; the gate Dropouts are applied inside from their seeds
        U, s_parts = (None, ops.panel_gate_score(h, views[1], views[3], views[4], bc, parts=True)) if route.gate == "fused" else \
            ops.panel_gate_u(h, views[1], views[3], views[4], bc, ka, kb, parts=True)
        # the epilogue's partial rows summed on the way, and the pooled rows cleared for the pass below: one launch
        M = torch.empty((B, L), dtype=torch.float32, device=h.device)
        s, A = ops.softmax_rows_parts(s_parts, B, N, zero=M)
        ops.weighted_rowsum(h.view(B, N, L), A.view(B, N, 1), into=M)
        return U, s, A, M
    wab, bab = (torch.cat([wa, wb], 0), torch.cat([ba, bb], 0)) if gated else (wa, ba)           # both gate branches, one pass
    if route.gate == "panel":        # bf16 with 512-wide h: the weight-stationary panel kernel (same GEMM, half the time of the tile kernel)
        U, _, _ = ops.panel_gemm(h, c(wab), ops.PG_BIAS, bias=bab)
    else:
        U = ops.gemm_nt(h, c(wab), epi=ops.EPI_BIAS, bias=bab)
    s = ops.gated_score_fwd(U, wc.reshape(-1).contiguous(), bc, ka, kb, gated=gated).view(B, N)
    A = ops.softmax_rows(s)
    return U, s, A, ops.weighted_rowsum(h.view(B, N, L), A.view(B, N, 1)).view(B, L)


def _clam_custom_inst_loss(custom_loss, logits_g, targets):
    """The reference hands (logits [rows,2], targets [rows]) of every evaluated (bag, class) pair to whatever loss it was constructed with
    (clam.py:118,131).  The gather, the classifier product and the predictions are the HIP kernels; the caller's loss runs on the pair's few
    logits as given (rows with target -1 do not exist for that pair) and its gradient w.r.t. them - taken here with autograd on that leaf - takes
    the place of the cross-entropy gradient in the backward pass.  A loss with parameters of its own gets no gradient for them.  -> (loss [B*n_cls], dlogits [B*n_cls*2k, 2])"""
    B, n_cls = targets.shape[:2]
    with torch.enable_grad():
        leaf = logits_g.detach().requires_grad_()
        pair = []
        for b_ in range(B):
            for c_ in range(n_cls):
                keep_rows = targets[b_, c_] >= 0
                pair.append(custom_loss(leaf[b_, c_][keep_rows], targets[b_, c_][keep_rows]) if bool(keep_rows.any()) else leaf.new_zeros(()))
        loss_pairs = torch.stack(pair).view(B, n_cls)
        dl_g, = torch.autograd.grad(loss_pairs.sum(), leaf, allow_unused=True)
    return loss_pairs.detach().reshape(-1), (torch.zeros_like(logits_g) if dl_g is None else dl_g).reshape(-1, 2).contiguous()


def _clam_inst_forward(route, h, A, inst_w, inst_b, inst_cfg, B, N):
    """Instance-level evaluation for ALL (bag, class) pairs at once (clam.py:103-132,150-168): the k top and k bottom patches of a bag
    are the same rows for every class, so one gather, one stacked classifier GEMM and one grouped cross-entropy launch replace the
    per-class / per-bag loops; pairs differ only in their targets (``_inst_constants``)
    -> (inst_loss [B], ids [B,2k], predictions / targets [2,B,n_cls,2k], what the backward needs)"""
    (labels, k, subtyping), dev, n_cls = inst_cfg[:3], h.device, inst_w.shape[0]
    ids = ops.topk_ids(A, k)
    lab = labels.to(device=dev, dtype=torch.int64) if isinstance(labels, torch.Tensor) else \
        torch.as_tensor([int(v) for v in labels], dtype=torch.int64).to(dev)
    w_st = inst_w.reshape(n_cls * 2, -1).contiguous()
    if route.inst_fused:
        # one launch: gather the 2k rows, all 2 n_cls instance logits, the cross-entropies and their gradients
        inst_loss, dl, inst_pt = ops.clam_inst_fwd(h, ids, lab, w_st, inst_b.reshape(-1), B, N, k, n_cls, subtyping)
        return inst_loss, ids, inst_pt, CLAMInstFused(ids, dl, w_st, k, n_cls)
    base, cls_ids, t_in, t_out = _inst_constants(dev, B, N, k, n_cls, subtyping)
    rows_all = (base + ids.to(torch.int64)).reshape(-1)                        # [B*2k] rows of h
    feats = ops.take_rows(h, rows_all)                                         # [B*2k, L] f32
    logits = ops.gemm_nt(feats, w_st, epi=ops.EPI_BIAS, bias=inst_b.reshape(-1).contiguous())   # [B*2k, 2 n_cls]
    logits_g = logits.view(B, 2 * k, n_cls, 2).permute(0, 2, 1, 3).contiguous()                 # [B, n_cls, 2k, 2]
    targets = torch.where((lab.view(B, 1) == cls_ids).unsqueeze(2), t_in, t_out).contiguous()   # [B, n_cls, 2k]
    loss_g, dl_g, preds_g = ops.cross_entropy(logits_g.view(-1, 2), targets.view(-1), 2 * k)
    if len(inst_cfg) > 3 and inst_cfg[3] is not None:                          # a caller-supplied instance_loss_fn (clam.py:64-65)
        loss_g, dl_g = _clam_custom_inst_loss(inst_cfg[3], logits_g, targets)
    scale = 1.0 / n_cls if subtyping else 1.0                                  # clam.py:167-168
    inst_pt = torch.stack([preds_g.view(B, n_cls, 2 * k), targets], 0)         # -1 where a pair has no such row
    return loss_g.view(B, n_cls).sum(1) * scale, ids, inst_pt, CLAMInstExplicit(rows_all, feats, dl_g, scale, k, n_cls)


def _clam_dgrad(route, x2, h, U, A, M, dM, m1, wa, wb, wc, ka, kb, wab_t, B, N):
    """Pooling, soft-max and gate backward, then dZ1 = (dU [Wa;Wb] + A (x) dM) * relu'(h) (h is already the dropped h: zero where dropped)
    -> (dU, dwc, dbc, column sums of dU, dWab or None, dz1, column sums of dz1 or None).  dWab None: the node's two big weight gradients
    wait for dz1 and share one grouped launch (``_clam_param_grads``), and dz1's column sums are its deferred partial rows - decided here only."""
    L, D, gated = h.shape[1], wa.shape[0], wb is not None
    if route.gate == "u":
        # pooling + soft-max + gate backward in ONE pass over (h, U): sum_m A_m (h_m . dM) = M . dM, so ds_n = A_n (h_n . dM - M . dM)
        # needs no reduction over the bag; U / dU - and wab_t [L, 2D] - in the interleaved column order of the forward
        dU, dwc, dbc, dbab = ops.gated_score_bwd_il(U, wc.reshape(-1).contiguous(), ka, kb, h=h, dM=dM, Mp=M, A=A.view(-1), rows_per_bag=N)
        # gate + first-layer weight gradients (clam.py:69-72) wait for dz1 and share one round of workgroups; the reduce launch
        # also undoes the 16-row interleave, applies the Dropout factor and sums the bias-gradient rows (no ATen launches)
        grouped = _GROUP_WGRAD and ops.gemm_tn_grouped_ok([(dU, h, None, None, None), (h, x2, None, None, None)])
        dwab = None if grouped else ops.gemm_tn(dU, h).view(D // 16, 2, 16, L).permute(1, 0, 2, 3).reshape(2 * D, L)   # rows back in [Wa; Wb] order
    else:
        dA = ops.rows_dot(h.view(B, N, L), dM.view(B, 1, L)).view(B, N)           # pooling: dA[n] = h[n].dM ; soft-max backward ; gate backward
        ds = ops.softmax_rows_bwd(A, dA).view(-1)
        dU, dwc, dbc, dbab = ops.gated_score_bwd(U, wc.reshape(-1).contiguous(), ds, ka, kb, gated=gated)   # dbab: column sums, same pass
        dwab = ops.gemm_tn(dU, h)                                                     # [2D, L] (gated) / [D, L]
        wab_t = ops.transpose_cast(torch.cat([wa, wb], 0) if gated else wa, h.dtype)
    if not route.dz1_panel:
        return dU, dwc, dbc, dbab, dwab, ops.gemm_nt(dU, wab_t, epi=ops.EPI_RANK1_MASK, mask=h, rowscale=A.view(-1), rank1=dM, rows_per_bag=N), None
    # column sums (the bias gradient) come out of the same launch; the instance branch extends them by the few rows it adds
    dz1, _, db1 = ops.panel_gemm(dU, wab_t, ops.PG_RANK1_MASK, bitmask=m1 if m1 is not None else ops.relu_bitmask(h),
                                 rowscale=A.view(-1), rank1=dM, rows_per_bag=N, colsum=True, colsum_defer=dwab is None)
    return dU, dwc, dbc, dbab, dwab, dz1, db1


def _clam_inst_backward(route, saved, h, dz1, dinst, inst_w, B, N, colsum_into):
    """Instance branch: classifier gradients, and the sparse feature gradients added into dz1 under the same ReLU mask.  The panel dz1 product took its
    column sums before these rows: theirs are added to ``colsum_into`` or, without one, returned -> (dW_inst [n_cls,2,L], db_inst [n_cls,2], those sums or None)."""
    k, n_cls = saved.k, saved.n_cls
    if route.inst_fused:
        dwi, dbi, gsum = ops.clam_inst_bwd(h, saved.ids, saved.w_st, saved.dl, dinst.float(), B, N, k, n_cls, dz1)
        if colsum_into is not None:
            colsum_into.add_(gsum)
    else:
        up = (dinst * saved.scale).view(B, 1, 1, 1)                                # upstream weight per (bag, ...)
        dlog = (saved.dl.view(B, n_cls, 2 * k, 2) * up).permute(0, 2, 1, 3).reshape(B * 2 * k, 2 * n_cls).contiguous()
        dwi = ops.gemm_tn(dlog, saved.feats)                                       # (gemm_tn pads narrow N1 itself)
        dbi = ops.colsum(dlog)
        g = ops.gemm_nt(dlog, inst_w.reshape(n_cls * 2, -1).t().contiguous())      # [B*2k, L]; K = 2 n_cls is padded
        ops.scatter_add_rows_masked(dz1, h, saved.rows, g, write_back=route.dz1_panel)
        gsum = ops.colsum(g, out=colsum_into, accumulate=colsum_into is not None) if route.dz1_panel else None   # of the rows just added
    return dwi.view(n_cls, 2, -1), dbi.view(n_cls, 2), None if colsum_into is not None else gsum


def _clam_param_grads(dU, h, dz1, x2, dwab, db1, inst_sums, k1):
    """-> (dW1, db1, dWab): the first layer's weight gradient - with the gate's in one grouped launch where that waited (``dwab`` None) - and
    its bias gradient from ``db1`` (``_clam_dgrad``) and ``inst_sums``, what the instance branch added behind deferred sums; the Dropout factor on both."""
    kp = None if k1 is None else k1.keep_q if isinstance(k1, ops.DropSeed) else 0.75      # the surviving entries of the keep mask all equal 1/0.75
    if dwab is None:
        parts, db1 = db1, torch.empty((h.shape[1],), dtype=torch.float32, device=dz1.device)
        dwab, dw1 = ops.gemm_tn_grouped([(dU, h, None, None, None, {"deinterleave": True}),
                                         (dz1, x2, None, db1, parts, dict({} if kp is None else {"scale": 1.0 / kp}, overwrite=True))], fresh=True)
        if inst_sums is not None:
            db1 = db1 + (inst_sums if kp is None else inst_sums / kp)
        return dw1, db1, dwab
    dw1 = ops.gemm_tn(dz1, x2)
    if db1 is None:
        db1 = ops.colsum(dz1)
    return (dw1, db1, dwab) if kp is None else (dw1 / kp, db1 / kp, dwab)


class CLAMFn(torch.autograd.Function):
    """CLAM_SB.bag_forward for a batch of equal-length bags, optionally with the instance-level loss (models/clam.py:134-181,103-132).
    x [B,N,d] in the compute dtype; parameters f32 (``wb`` / ``bb`` None: the plain ``Attn_Net`` of ``CLAM_SB(gate=False)``, clam.py:18-34,80-81).
    ``keeps`` = None (eval) or the Dropout keeps of h, the tanh branch and the sigmoid branch (clam.py:71-72,47-48): three ``ops.DropSeed``s,
    or three keep-multiplier tensors (values 0 or 1/0.75; parity tests).  ``inst_cfg`` = None or (labels: list[int] or tensor [B], k_sample,
    subtyping[, instance_loss_fn]) with ``inst_w`` [n_cls,2,L], ``inst_b`` [n_cls,2]; ``grad_on``: see ABMILFn.forward.

    ``clam_route`` picks every form once, in ``forward``; ``backward`` reads the stored route:
      first layer  ``ops.panel_gemm`` (bf16, d = 512) or ``ops.gemm_nt``; its Dropout in that epilogue (panel kernel, seeds), in
                   ``ops.dropout_relu_bitmask`` (seeds, B*N % 32 == 0), by ``ops.mul`` with an ``ops.dropout_mask`` or the caller's tensor;
      gate         fused (bf16, L = 2D = 512, eval, no backward to follow): ``ops.panel_gate_score``, no pre-activations;
                   u (the same shapes, no keep tensors, ``ops.gated_bwd_il_supported``): ``ops.panel_gate_u``, backward in one pass
                   (``ops.gated_score_bwd_il``); both pool by ``ops.softmax_rows_parts`` + ``ops.weighted_rowsum(into=)``;
                   panel / tile (``gate=False``, ``size_arg="big"``, keep tensors, f32): ``ops.panel_gemm`` or ``ops.gemm_nt``, then
                   ``gated_score_fwd``, ``softmax_rows``, ``weighted_rowsum``; ``rows_dot``, ``softmax_rows_bwd``, ``gated_score_bwd`` back;
      dz1          ``ops.panel_gemm(PG_RANK1_MASK)`` with its column sums (bf16, 512 gate columns) or ``ops.gemm_nt(EPI_RANK1_MASK)``;
                   behind gate u the two big weight gradients go as one ``ops.gemm_tn_grouped`` where its plan groups them;
      instance     one launch each way (``ops.clam_inst_fwd`` / ``clam_inst_bwd``: the default cross-entropy, n_cls <= 8, k <= 32), or
                   ``take_rows``, ``gemm_nt``, ``cross_entropy`` [, the caller's loss on the host] and ``scatter_add_rows_masked`` back.
    Returns (M [B,L], A [B,N], raw scores [B,N], inst_loss [B], ids [B,2k] int32, [2,B,n_cls,2k] int64: predictions and targets per (bag,
    class), -1 where a pair has no such row); without ``inst_cfg`` the last three are zeros / empty.  Only M and inst_loss carry grad."""

    @staticmethod
    def forward(ctx, x, w1, b1, wa, ba, wb, bb, wc, bc, inst_w, inst_b, keeps, inst_cfg, grad_on=True):
        (B, N, d), T, dev = x.shape, x.dtype, x.device
        k1, ka, kb = keeps if keeps is not None else (None, None, None)
        # bf16 gated chain: the compute-dtype copy of fc, the two gate Linears interleaved for the panel kernel and their transpose
        # come out of ONE launch (none between optimizer steps) instead of a dozen cat / gather / cast launches - ahead of the route, whose
        # queries then run beside it (30 us more from an idle GPU to the first launch measured the other way round)
        views = ops.clam_views(w1, wa, ba, wb, bb, wc, T) if (T == torch.bfloat16 and wb is not None and wa.shape[0] % 16 == 0) else None
        route = clam_route(B, N, d, w1.shape[0], wa.shape[0], T, wb is not None,
                           None if keeps is None else "seeds" if isinstance(k1, ops.DropSeed) else "tensors", bool(grad_on), any(ctx.needs_input_grad),
                           None if inst_cfg is None else (inst_w.shape[0], inst_cfg[1], len(inst_cfg) > 3 and inst_cfg[3] is not None))
        x2 = x.reshape(B * N, d)
        c = (lambda w: views[0] if w is w1 else ops.cast(w, T)) if views is not None else (lambda w: w) if T == torch.float32 else (lambda w: ops.cast(w, T))
        h, m1 = _clam_first_layer(route, x2, c(w1), b1, k1)
        U, s, A, M = _clam_gate(route, h, B, N, (wa, ba, wb, bb, wc, bc), views, c, ka, kb)
        if inst_cfg is not None:
            inst_loss, ids, inst_pt, saved_inst = _clam_inst_forward(route, h, A, inst_w, inst_b, inst_cfg, B, N)
        else:
            # the cached zero is shared by every call without an instance branch: as a differentiable output autograd would re-point its
            # grad_fn at this node (keeping the node's saved activations alive through the cache) - hand out a view, marked non-differentiable
            inst_loss, saved_inst = _zeros_const(dev, B).detach()[:], None
            ids, inst_pt = torch.zeros((B, 0), dtype=torch.int32, device=dev), torch.zeros((2, B, 0, 0), dtype=torch.int64, device=dev)
        ctx.save_for_backward(x2, h, U if U is not None else _placeholder(x2), A, M, w1, wa, wb, wc,
                              inst_w if inst_w is not None else _placeholder(x2), m1)
        ctx.bias_params = (b1, ba, bb, bc)               # (the parameters themselves: the backward pass adds into their gradient buffers)
        ctx.wab_t = views[2] if route.gate == "u" else None   # (a cached view: parameters do not change between a forward and its backward)
        ctx.route, ctx.keeps, ctx.saved_inst, ctx.dims = route, keeps, saved_inst, (B, N)
        ctx.mark_non_differentiable(A, s, ids, inst_pt, *((inst_loss,) if inst_cfg is None else ()))
        ctx.set_materialize_grads(False)
        return M, A, s, inst_loss, ids, inst_pt

    @staticmethod
    def backward(ctx, dM, _dA, _ds, dinst, _dids, _dpt):
        _enter(ctx)
        x2, h, U, A, M, w1, wa, wb, wc, inst_w, m1 = ctx.saved_tensors
        (b1, ba, bb, bc), route, (B, N), D = ctx.bias_params, ctx.route, ctx.dims, wa.shape[0]
        k1, ka, kb = ctx.keeps if ctx.keeps is not None else (None, None, None)
        dM = dM.contiguous() if dM is not None else torch.zeros_like(M)
        dU, dwc, dbc, dbab, dwab, dz1, db1 = _clam_dgrad(route, x2, h, U, A, M, dM, m1, wa, wb, wc, ka, kb, ctx.wab_t, B, N)
        dinst_w = dinst_b = inst_sums = None
        if ctx.saved_inst is not None and dinst is not None:
            dinst_w, dinst_b, inst_sums = _clam_inst_backward(route, ctx.saved_inst, h, dz1, dinst, inst_w, B, N, None if dwab is None else db1)
        dw1, db1, dwab = _clam_param_grads(dU, h, dz1, x2, dwab, db1, inst_sums, k1)
        gate = [(dwab, wa), (dbab.contiguous(), ba)] if wb is None else \
            [(dwab[:D].contiguous(), wa), (dbab[:D].contiguous(), ba), (dwab[D:].contiguous(), wb), (dbab[D:].contiguous(), bb)]
        # the eight (six without the gate) parameter gradients: added to the optimizer's pre-seated buffers by ONE launch (autograd's
        # AccumulateGrad would run one ATen add per parameter); parameters without such a buffer get their tensors back
        dw1, db1, *dgate, dwc, dbc = _pgrads((dw1, w1), (db1, b1), *gate, (dwc.view(1, -1), wc), (dbc, bc))
        return (None, dw1, db1, *dgate, *([None, None] if wb is None else []), dwc, dbc, dinst_w, dinst_b, None, None, None)


class PolicyHeadFn(torch.autograd.Function):
    """log-prob of given actions under N(sigmoid(z), diag(std)) (ActorCritic.evaluate, rlmil.py:115-121)."""

    @staticmethod
    def forward(ctx, z, actions, std):
        mu, act, logp = ops.policy_head_fwd(z, std, actions=actions)
        ctx.save_for_backward(mu, act)
        ctx.std = std
        return logp

    @staticmethod
    def backward(ctx, dlogp):
        mu, act = ctx.saved_tensors
        return ops.policy_head_bwd(mu, act, dlogp, ctx.std), None, None


class PPOLossFn(torch.autograd.Function):
    """mean(-min(surr1, surr2) + 0.5*MSE - 0.01*entropy) (PPO.update, rlmil.py:172-181)."""

    @staticmethod
    def forward(ctx, logp, old_logp, value, ret, eps_clip, entropy, n_total=None):
        loss, dlogp, dvalue = ops.ppo_loss(logp, old_logp, value, ret, eps_clip, entropy, n_total)
        ctx.save_for_backward(dlogp, dvalue)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dlogp, dvalue = ctx.saved_tensors
        return dlogp * g, None, dvalue * g, None, None, None, None


class GroupedCrossEntropyFn(torch.autograd.Function):
    """Mean CE of every group of ``group`` consecutive rows of [R,C] logits -> [R/group] losses, one launch: the T per-patch-step
    ``nn.CrossEntropyLoss()`` values of a step whose T x B head rows were computed together (train_RLMIL.py:316,502,709).  With
    ``want_conf`` -> (losses, conf [R]): the soft-max confidence of each row's true class from the same launch (the RL-MIL rewards
    are its differences between patch steps, train_RLMIL.py:345,369-371); conf is not differentiable."""

    @staticmethod
    def forward(ctx, logits, targets, group, want_conf=False):
        res = ops.cross_entropy(logits.float().contiguous(), targets.to(torch.int64).contiguous(), int(group), want_conf=bool(want_conf))
        ctx.save_for_backward(res[1])
        ctx.group = int(group)
        if want_conf:
            ctx.mark_non_differentiable(res[3])
            return res[0], res[3]
        return res[0]

    @staticmethod
    def backward(ctx, g, _gconf=None):
        (dl,) = ctx.saved_tensors
        return dl * g.reshape(-1, 1).repeat_interleave(ctx.group, 0), None, None, None


class StepCEMeanFn(torch.autograd.Function):
    """The loss of a supervised RL-MIL step whose T x B head rows were computed together (train_RLMIL.py:316,502,709 per patch step,
    their mean over the T steps as the step loss): logits [T*B, C], targets [T*B] -> (mean_t loss_t, loss_t [T], conf [T*B]) with
    loss_t = nn.CrossEntropyLoss() of step t's B rows and conf the soft-max confidence of each row's true class (the rewards are its
    differences between steps, :345,369-371).  One cross-entropy launch + one mean launch forward, ONE scaling of the stored
    d(loss_t)/d(logits) backward; loss_t and conf are not differentiable (a sum / division node over loss_t, a repeat_interleave and a
    multiply in the backward pass were ~10 ATen launches per step)."""

    @staticmethod
    def forward(ctx, logits, targets, group):
        loss_t, dl, _, conf = ops.cross_entropy(logits.float().contiguous(), targets.to(torch.int64).contiguous(), int(group), want_conf=True)
        ctx.save_for_backward(dl)
        ctx.T = loss_t.numel()
        ctx.mark_non_differentiable(loss_t, conf)
        ctx.set_materialize_grads(False)
        return ops.mean_small(loss_t), loss_t, conf

    @staticmethod
    def backward(ctx, g, _gl=None, _gc=None):
        (dl,) = ctx.saved_tensors
        if g is None:
            return None, None, None
        if ops.is_unit_grad(g):
            return ops.axpby(dl, dl, 1.0 / ctx.T, 0.0), None, None
        return dl * (g / ctx.T), None, None


class StepLossFn(torch.autograd.Function):
    """``StepCEMeanFn`` for the two architectures whose step loss mixes a second term into the head's cross-entropy
    (train_RLMIL.py:336 CLAM-SB: ``bag_weight * ce + (1 - bag_weight) * instance_loss``, the instance loss averaged over the B bags of
    the step; :527-529 DSMIL: ``0.5 * ce + 0.5 * ce(max-instance scores)``): logits [T*B, C], targets [T*B], ``extra`` = the per-bag
    instance losses [T*B] (``extra_is_logits`` False) or the second logits [T*B, C'] -> (mean_t loss_t, loss_t [T], conf [T*B]).
    Forward: the cross-entropy launch(es), a grouped mean, one mixing launch, one mean launch; backward: one scaling per input (the
    instance-loss gradient is a constant).  ``loss_t`` and ``conf`` are not differentiable."""

    @staticmethod
    def forward(ctx, logits, targets, group, w_ce, extra, w_x, extra_is_logits):
        tg = targets.to(torch.int64).contiguous()
        ce_t, dl, _, conf = ops.cross_entropy(logits.float().contiguous(), tg, int(group), want_conf=True)
        T_ = ce_t.numel()
        if extra_is_logits:
            x_t, dlx, _ = ops.cross_entropy(extra.float().contiguous(), tg, int(group))
            ctx.save_for_backward(dl, dlx)
        else:
            x_t = ops.group_mean(extra.float().contiguous().view(-1), T_, int(group))
            ctx.save_for_backward(dl)
        loss_t = ops.axpby(ce_t, x_t, float(w_ce), float(w_x))
        ctx.meta = (T_, int(group), float(w_ce), float(w_x), bool(extra_is_logits), tuple(extra.shape))
        ctx.mark_non_differentiable(loss_t, conf)
        ctx.set_materialize_grads(False)
        return ops.mean_small(loss_t), loss_t, conf

    @staticmethod
    def backward(ctx, g, _gl=None, _gc=None):
        if g is None:
            return (None,) * 7
        T_, group, w_ce, w_x, is_logits, xshape = ctx.meta
        dl = ctx.saved_tensors[0]
        if ops.is_unit_grad(g):
            dlogits = ops.axpby(dl, dl, w_ce / T_, 0.0)
            if is_logits:
                dlx = ctx.saved_tensors[1]
                dextra = ops.axpby(dlx, dlx, w_x / T_, 0.0)
            else:
                dextra = ops.filled(xshape, w_x / (T_ * group), dl.device)
        else:
            dlogits = dl * (g * (w_ce / T_))
            dextra = ctx.saved_tensors[1] * (g * (w_x / T_)) if is_logits else (g * (w_x / (T_ * group))).expand(xshape).contiguous()
        return dlogits, None, None, None, dextra, None, None


class CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss() (mean) over [R,C] logits (train_RLMIL.py:316,502,709)."""

    @staticmethod
    def forward(ctx, logits, targets):
        loss, dl, preds = ops.cross_entropy(logits.float().contiguous(), targets.to(torch.int64).contiguous(), logits.shape[0])
        ctx.save_for_backward(dl)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None
