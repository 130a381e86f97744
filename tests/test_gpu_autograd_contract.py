"""One contract across the model paths: a gradient obtained through a different autograd route equals the plain-backward gradient,
and that plain gradient matches a high-precision reference.

Routes: (1) plain ``backward()`` against the CPU oracle; (2) saved-tensor hooks that copy what autograd saves (``save_on_cpu``, a
clone); (3) activation checkpointing, with training-mode Dropout included (the recomputation must apply the masks the forward drew);
(4) partial backward with direct gradient accumulation on (a ``FlatAdam`` seats every ``.grad``): ``backward(inputs=...)`` and
``autograd.grad`` leave every ``p.grad`` as it was, while plain ``backward()`` still accumulates straight into the flat buffer;
(5) forward-only calls under ``no_grad`` / ``inference_mode``.

Routes 2-4 run the same kernels on the same inputs as route 1.  ``_same`` compares them bit for bit except where a launch adds its
partial results with float atomics, whose order varies from run to run: there the bound is 2e-6 of the largest entry on the f32
paths, 5e-4 on the bf16 paths (a reordered f32 sum upstream can move a gradient that is stored as bf16 by one bf16 ulp) - far below
what a misread weight layout or a mismatched dropout mask does (both move gradients by O(1) of their size).
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detrand, mil_oracle as O, params as P

pytestmark = pytest.mark.gpu

T = torch.from_numpy
BF16 = torch.bfloat16
F32 = torch.float32


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _r16(t):
    return t.bfloat16().float()


# ---------------------------------------------------------------- the paths
class Case:
    """A model path: ``build()`` a fresh module on the device from the oracle's parameters, its ``inputs()``, and ``fwd(m, inp)`` ->
    (loss, output).  ``xin(inp)`` is the input whose gradient the partial routes ask for (the patch features where the module
    differentiates them, otherwise the weight of the loss).  ``direct``: plain backward under a FlatAdam adds gradients straight
    into the flat buffer on this path (the general ABMIL backward returns every gradient to autograd instead)."""

    def __init__(self, name, build, inputs, fwd, xin, oracle, direct=True, seed=0):
        self.name, self.build, self.inputs, self.fwd, self.xin, self.oracle = name, build, inputs, fwd, xin, oracle
        self.direct, self.seed = direct, seed


def _grads(m):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _check_f32(got, want, key, rtol=1e-3, atol=2e-4):
    """f32 kernels vs the f32 oracle: the tolerances of tests/test_gpu_modules.py test_abmil_vs_oracle_full_grads."""
    want = want.detach().double()
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), want.numpy(), rtol=rtol,
                               atol=atol * max(want.abs().max().item(), 1e-30), err_msg=key)


def _check_norm(got, want, key, rel):
    """bf16 storage vs an f32 oracle: norm-wise, as the bf16-vs-f32 module tests."""
    got, want = got.detach().double().cpu(), want.detach().double()
    err = ((got - want).norm() / want.norm().clamp_min(1e-30)).item()
    assert err < rel, (key, err)


# -- ABMIL
def _abmil_build(L=512, D=128, dtype=F32, dropout=0.0, seed=3):
    def build():
        from murcl_amd.models.abmil import ABMIL
        m = ABMIL(512, L=L, D=D, dim_out=128, dropout=dropout)
        m.load_state_dict(P.to_torch(P.abmil(seed, L=L, D=D)))
        m.compute_dtype = dtype
        return m.to(_dev()).train()
    return build


def _abmil_inputs(B, N, L, dtype, seed):
    def inputs():
        x = T(P.bags(seed, f"ac.x{B}.{N}", B, N, 512)).to(_dev()).to(dtype).requires_grad_()
        w = T(detrand.normal(seed, f"ac.w{L}", (B, L))).to(_dev())
        return x, w
    return inputs


def _abmil_fwd(m, inp):
    x, w = inp
    out, _ = m(x)
    return (out * w).sum(), out


def _abmil_masks(case, B, N, L, dtype):
    """The two keep masks the module draws after ``torch.manual_seed(case.seed)`` (its first two draws off the CPU generator),
    materialised: [B,N,L], 0 or the realised 1/keep."""
    from murcl_amd import ops
    torch.manual_seed(case.seed)
    seeds = (ops.dropout_seed(), ops.dropout_seed())
    return [ops.dropout_mask((B * N, L), dtype, 0.75, _dev(), seed=s).float().reshape(B, N, L).cpu() for s in seeds]


def _abmil_oracle_f32(B, N, L, D, dropout, seed):
    def oracle(case, got_out, got, got_x):
        p = {k: v.clone().requires_grad_() for k, v in P.to_torch(P.abmil(seed, L=L, D=D)).items()}
        x, w = (t.detach().cpu() for t in case.inputs())
        x.requires_grad_()
        masks = _abmil_masks(case, B, N, L, F32) if dropout else None
        out, _, _, _ = O.abmil_forward(p, x, masks)
        (out * w).sum().backward()
        _check_f32(got_out, out, "out", rtol=1e-4, atol=1e-5)
        _check_f32(got_x, x.grad, "dx")
        for k, v in got.items():
            if p[k].grad is None:                                 # (ABMIL.fc: built, never applied)
                assert v is None, k
            elif k != "attention.2.bias":                         # (a soft-max shift: exactly zero in exact arithmetic)
                _check_f32(v, p[k].grad, k)
    return oracle


def _abmil_oracle_bf16_storage(B, N, seed):
    """The f32 oracle with the bf16 path's storage roundings inserted (tests/test_gpu_modules.py
    test_bf16_backward_against_the_oracle_with_the_same_storage_roundings): every parameter gradient within 2e-3 of its largest
    entry; the input gradient (the HIP path stores it as bf16) within 1e-2 norm-wise."""
    def oracle(case, got_out, got, got_x):
        p = {k: v.clone().requires_grad_() for k, v in P.to_torch(P.abmil(seed)).items()}
        x, w = (t.detach().cpu().float() for t in case.inputs())
        x.requires_grad_()

        def st(t):                                   # round forward, identity backward
            return t + (_r16(t) - t).detach()

        def grad_r16(t):                             # the gradient arriving at t is stored as bf16
            t.register_hook(lambda g: _r16(g))
            return t
        h = x
        for k in ("encoder.0", "encoder.3", "encoder.6"):
            z = grad_r16(F.linear(h, st(p[k + ".weight"]))) + p[k + ".bias"]
            h = st(torch.relu(z))
        t_pre = grad_r16(F.linear(h, st(p["attention.0.weight"]))) + p["attention.0.bias"]
        s = F.linear(torch.tanh(t_pre), p["attention.2.weight"], p["attention.2.bias"]).squeeze(-1)
        A = torch.softmax(s, 1) / math.sqrt(N)
        M = torch.einsum("bn,bnl->bl", A, h)
        out = torch.relu(F.linear(M, p["decoder.0.weight"], p["decoder.0.bias"]))
        (out * w).sum().backward()
        assert (got_out.detach().cpu() - out).abs().max().item() <= 1e-4 * out.abs().max().item()
        _check_norm(got_x, x.grad, "dx", 1e-2)
        for k, v in got.items():
            if v is None or k == "attention.2.bias":
                continue
            ref = p[k].grad
            err = (v.cpu() - ref).abs().max().item() / ref.abs().max().item()
            assert err <= 2e-3, (k, err)
    return oracle


def _abmil_oracle_bf16_dropout(B, N, seed):
    """bf16 fast path with training-mode Dropout against the f32 oracle fed the same masks: the bf16-vs-f32 bounds of
    test_abmil_dropout_bf16_fast_path_close_to_fp32_and_seeded_masks_equal_materialised_ones."""
    def oracle(case, got_out, got, got_x):
        p = {k: v.clone().requires_grad_() for k, v in P.to_torch(P.abmil(seed)).items()}
        x, w = (t.detach().cpu().float() for t in case.inputs())
        x.requires_grad_()
        out, _, _, _ = O.abmil_forward(p, x, _abmil_masks(case, B, N, 512, BF16))
        (out * w).sum().backward()
        assert (got_out.detach().cpu() - out).abs().max().item() <= 3e-2 * out.abs().max().item()
        # (the input gradient is a cancelling sum over L: the bf16 roundings of dZ1 and of the masks weigh more than in the
        # parameter gradients; a wrong mask or weight layout is O(1))
        _check_norm(got_x, x.grad, "dx", 1e-1)
        for k, v in got.items():
            if v is not None and k != "attention.2.bias":
                _check_norm(v, p[k].grad, k, 6e-2)
    return oracle


def _abmil_case(name, B, N, L=512, D=128, dtype=F32, dropout=0.0, seed=3, oracle=None, direct=True):
    if oracle is None:
        oracle = _abmil_oracle_f32(B, N, L, D, dropout, seed)
    return Case(name, _abmil_build(L, D, dtype, dropout, seed), _abmil_inputs(B, N, L, dtype, seed), _abmil_fwd,
                lambda inp: inp[0], oracle, direct=direct, seed=seed)


# -- CLAM_SB (gated, small), with the instance loss
def _clam_build(dtype, train, seed):
    def build():
        from murcl_amd.models.clam import CLAM_SB
        m = CLAM_SB(gate=True, size_arg="small", dropout=True, k_sample=8, n_classes=2, subtyping=False, in_dim=512)
        m.load_state_dict(P.to_torch(P.clam_sb(seed)))
        m.compute_dtype = dtype
        return m.to(_dev()).train(train)
    return build


CLAM_LABELS = [1, 0]


def _clam_inputs(B, N, dtype, seed):
    def inputs():
        x = T(P.bags(seed, "cc.x", B, N, 512)).to(_dev()).to(dtype)
        w = T(detrand.normal(seed, "cc.w", (B, 512))).to(_dev()).requires_grad_()
        return x, w
    return inputs


def _clam_fwd(m, inp):
    x, w = inp
    M, _, res = m(x, label=CLAM_LABELS, instance_eval=True)
    return (M * w).sum() + sum(r["instance_loss"] for r in res), M


def _clam_oracle(B, N, dtype, train, seed):
    def oracle(case, got_out, got, got_w):
        from murcl_amd import ops
        p = {k: v.clone().requires_grad_() for k, v in P.to_torch(P.clam_sb(seed)).items()}
        x, w = (t.detach().cpu().float() for t in case.inputs())
        w.requires_grad_()
        masks = None
        if train:                                    # the three Dropout(0.25) masks the module draws first (fc, gate a, gate b): 0 / 1
            torch.manual_seed(case.seed)
            seeds = [ops.dropout_seed() for _ in range(3)]
            masks = [(ops.dropout_mask((B * N, n), F32, 0.75, _dev(), seed=s) != 0).float().reshape(B, N, n).cpu()
                     for s, n in zip(seeds, (512, 256, 256))]
        M, A, _, h = O.clam_sb_forward(p, x, drop_mask=masks)
        loss = (M * w).sum() + sum(O.clam_instance_eval(p, A[b], h[b], CLAM_LABELS[b], 2, 8, False)[0] for b in range(B))
        loss.backward()
        if dtype == F32:
            _check_f32(got_out, M, "M", rtol=2e-4, atol=1e-5)
            _check_f32(got_w, w.grad, "dw", rtol=2e-4, atol=1e-5)
        else:
            _check_norm(got_out, M, "M", 3e-2)
            _check_norm(got_w, w.grad, "dw", 3e-2)
        for k, v in got.items():
            if p[k].grad is None or k.endswith("attention_c.bias"):
                continue
            if dtype == F32:
                _check_f32(v, p[k].grad, k, rtol=2e-3, atol=3e-4)
            else:
                _check_norm(v, p[k].grad, k, 6e-2)
    return oracle


def _clam_case(name, dtype, train, B=2, N=256, seed=12):
    return Case(name, _clam_build(dtype, train, seed), _clam_inputs(B, N, dtype, seed), _clam_fwd, lambda inp: inp[1],
                _clam_oracle(B, N, dtype, train, seed), seed=seed)


# -- DSMIL with the value branch's Dropout in training mode
def _dsmil_build(dtype, seed):
    def build():
        from murcl_amd.models.dsmil import BClassifier, FCLayer, MILNet
        m = MILNet(FCLayer(512, 2), BClassifier(512, 2, dropout_v=0.25))
        m.load_state_dict(P.to_torch(P.dsmil(seed, 512, 2)))
        m.compute_dtype = dtype
        return m.to(_dev()).train()
    return build


def _dsmil_inputs(B, N, dtype, seed):
    def inputs():
        x = T(P.bags(seed, "dc.x", B, N, 512)).to(_dev()).to(dtype)
        wb = T(detrand.normal(seed, "dc.wb", (B, 2, 512))).to(_dev()).requires_grad_()
        wc = T(detrand.normal(seed, "dc.wc", (B, N, 2))).to(_dev())
        return x, wb, wc
    return inputs


def _dsmil_fwd(m, inp):
    x, wb, wc = inp
    classes, bag, _ = m(x)
    return (bag * wb).sum() + (torch.stack(classes) * wc).sum(), bag


def _dsmil_oracle(B, N, dtype, seed):
    def oracle(case, got_out, got, got_wb):
        from murcl_amd import ops
        p = {k: v.clone().requires_grad_() for k, v in P.to_torch(P.dsmil(seed, 512, 2)).items()}
        x, wb, wc = (t.detach().cpu().float() for t in case.inputs())
        wb.requires_grad_()
        torch.manual_seed(case.seed)
        keep = ops.dropout_mask((B, N, 512), dtype, 0.75, _dev(), seed=ops.dropout_seed()).float().cpu()
        c, bag, _, _ = O.dsmil_forward(p, x, keep_v=keep)
        ((bag * wb).sum() + (c * wc).sum()).backward()
        if dtype == F32:
            _check_f32(got_out, bag, "bag", rtol=1e-4, atol=1e-5)
            _check_f32(got_wb, wb.grad, "dwb", rtol=1e-4, atol=1e-5)
        else:
            _check_norm(got_out, bag, "bag", 3e-2)
            _check_norm(got_wb, wb.grad, "dwb", 3e-2)
        for k, v in got.items():
            if p[k].grad is None:
                assert v is None, k
                continue
            if dtype == F32:
                _check_f32(v, p[k].grad, k, rtol=2e-3, atol=3e-4)
            else:
                _check_norm(v, p[k].grad, k, 6e-2)
    return oracle


def _dsmil_case(name, dtype, B=2, N=300, seed=23):
    return Case(name, _dsmil_build(dtype, seed), _dsmil_inputs(B, N, dtype, seed), _dsmil_fwd, lambda inp: inp[1],
                _dsmil_oracle(B, N, dtype, seed), seed=seed)


# -- CL(ABMIL) + Full_layer + NT_Xent: the pre-training loss (train_MuRCL.py:233-291, one patch step)
def _cl_build(seed=985):
    def build():
        from murcl_amd.models.abmil import ABMIL
        from murcl_amd.models.cl import CL
        from murcl_amd.models.rlmil import Full_layer
        enc = ABMIL(512, L=512, D=128, dim_out=128)
        enc.load_state_dict(P.to_torch(P.abmil(seed)))
        fc = Full_layer(512, 1024, True, 128)
        fc.load_state_dict(P.to_torch(P.full_layer(seed)))
        return torch.nn.ModuleDict({"model": CL(enc, 128, 512), "fc": fc}).to(_dev())
    return build


def _cl_inputs(B, N, seed):
    def inputs():
        return tuple(T(P.bags(seed, f"cl.{v}", B, N, 512)).to(_dev()).requires_grad_() for v in range(2))
    return inputs


def _cl_fwd(m, inp):
    from murcl_amd.utils.losses import NT_Xent
    outs, _ = m["model"](list(inp))
    z = [m["fc"](o, restart=True) for o in outs]
    return NT_Xent(z[0].shape[0], 1.0)(z[0], z[1]), torch.cat(z)


def _cl_oracle(seed):
    def oracle(case, got_out, got, got_x):
        mp = {k: v.clone().requires_grad_() for k, v in P.to_torch(P.abmil(seed)).items()}
        fp = {k: v.clone().requires_grad_() for k, v in P.to_torch(P.full_layer(seed)).items()}
        xs = [t.detach().cpu().requires_grad_() for t in case.inputs()]
        loss, *_ = O.pretrain_step(mp, fp, [xs], 1.0)
        loss.backward()
        _check_f32(got_x, xs[0].grad, "dx0")
        ref = {"model.encoder." + k: v.grad for k, v in mp.items()}
        ref.update({"fc." + k: v.grad for k, v in fp.items()})
        for k, v in got.items():
            if ref[k] is None or k.endswith("attention.2.bias"):
                continue
            _check_f32(v, ref[k], k)
    return oracle


# -- Full_layer: two GRU steps on one shared hidden state (restart, then continue)
def _gru_build(seed=985):
    def build():
        from murcl_amd.models.rlmil import Full_layer
        fc = Full_layer(512, 1024, True, 128)
        fc.load_state_dict(P.to_torch(P.full_layer(seed)))
        return fc.to(_dev())
    return build


def _gru_inputs(seed):
    def inputs():
        xs = [T(detrand.normal(seed, f"gc.x{t}", (8, 512))).to(_dev()).requires_grad_() for t in range(2)]
        ws = [T(detrand.normal(seed, f"gc.w{t}", (8, 128))).to(_dev()) for t in range(2)]
        return xs[0], xs[1], ws[0], ws[1]
    return inputs


def _gru_fwd(m, inp):
    x0, x1, w0, w1 = inp
    z0 = m(x0, restart=True)
    z1 = m(x1)
    return (z0 * w0).sum() + (z1 * w1).sum(), torch.cat([z0, z1])


def _gru_oracle(seed):
    def oracle(case, got_out, got, got_x):
        fp = {k: v.clone().requires_grad_() for k, v in P.to_torch(P.full_layer(seed)).items()}
        x0, x1, w0, w1 = (t.detach().cpu() for t in case.inputs())
        x0.requires_grad_()
        z0, h = O.full_layer_step(fp, x0, None)
        z1, _ = O.full_layer_step(fp, x1, h)
        ((z0 * w0).sum() + (z1 * w1).sum()).backward()
        _check_f32(got_out, torch.cat([z0, z1]), "z", rtol=1e-4, atol=1e-5)
        _check_f32(got_x, x0.grad, "dx0")
        for k, v in got.items():
            _check_f32(v, fp[k].grad, k)
    return oracle


# -- Full_layer over row blocks as one recurrent node: a rollout (forward_sequence) and the view sequence of a contrastive step
def _gru_blocks_inputs(seed, n):
    def inputs():
        x = T(detrand.normal(seed, f"gb.x{n}", (n * 8, 512))).to(_dev()).requires_grad_()
        return x, T(detrand.normal(seed, f"gb.w{n}", (n * 8, 128))).to(_dev())
    return inputs


def _gru_seq_fwd(m, inp):
    x, w = inp
    z = m.forward_sequence(x.view(-1, 8, 512))
    return (z * w).sum(), z


def _gru_view_seq_fwd(m, inp):
    x, w = inp
    z = m.forward_view_sequence(list(x.split(8, 0)))
    return (z * w).sum(), z


def _gru_blocks_oracle(seed, n, zero_blocks):
    """``O.full_layer_step`` block by block: the first ``zero_blocks`` from the zero state, block k from block k-1."""
    def oracle(case, got_out, got, got_x):
        fp = {k: v.clone().requires_grad_() for k, v in P.to_torch(P.full_layer(seed)).items()}
        x, w = (t.detach().cpu() for t in case.inputs())
        x.requires_grad_()
        zs, h = [], None
        for k in range(n):
            z, h = O.full_layer_step(fp, x[k * 8:(k + 1) * 8], None if k < zero_blocks else h)
            zs.append(z)
        z = torch.cat(zs)
        (z * w).sum().backward()
        _check_f32(got_out, z, "z", rtol=1e-4, atol=1e-5)
        _check_f32(got_x, x.grad, "dx")
        for k, v in got.items():
            _check_f32(v, fp[k].grad, k)
    return oracle


CASES = {c.name: c for c in [
    _abmil_case("abmil_f32", 2, 300),
    # the bf16 fast path: d = L = 512, D = 128 at a row count the weight-stationary kernels take -> fragment-order weight views
    _abmil_case("abmil_bf16", 4, 2048, dtype=BF16, seed=8, oracle=_abmil_oracle_bf16_storage(4, 2048, 8)),
    _abmil_case("abmil_dropout_f32", 2, 256, dropout=0.25, seed=5, direct=False),
    # the fast path's forward with Dropout: fragment-order views AND the general backward
    _abmil_case("abmil_dropout_bf16", 4, 2048, dtype=BF16, dropout=0.25, seed=9, oracle=_abmil_oracle_bf16_dropout(4, 2048, 9),
                direct=False),
    _abmil_case("abmil_L256_D64", 2, 200, L=256, D=64, seed=4, direct=False),
    _clam_case("clam_f32", F32, train=False),
    _clam_case("clam_f32_dropout", F32, train=True),
    _clam_case("clam_bf16_dropout", BF16, train=True),
    _dsmil_case("dsmil_f32_dropout_v", F32),
    _dsmil_case("dsmil_bf16_dropout_v", BF16),
    Case("cl_ntxent", _cl_build(), _cl_inputs(4, 256, 985), _cl_fwd, lambda inp: inp[0], _cl_oracle(985), seed=985),
    Case("full_layer_gru", _gru_build(13), _gru_inputs(13), _gru_fwd, lambda inp: inp[0], _gru_oracle(13), seed=13),
    Case("full_layer_seq", _gru_build(14), _gru_blocks_inputs(14, 3), _gru_seq_fwd, lambda inp: inp[0], _gru_blocks_oracle(14, 3, 1),
         seed=14),
    Case("full_layer_view_seq", _gru_build(15), _gru_blocks_inputs(15, 6), _gru_view_seq_fwd, lambda inp: inp[0],
         _gru_blocks_oracle(15, 6, 2), seed=15),
]}
NAMES = list(CASES)
HAS_DROPOUT = {"abmil_dropout_f32", "abmil_dropout_bf16", "clam_f32_dropout", "clam_bf16_dropout", "dsmil_f32_dropout_v",
               "dsmil_bf16_dropout_v"}


# ---------------------------------------------------------------- running a route
def _tol(name):
    return 5e-4 if "bf16" in name else 2e-6


SHIFT_BIASES = ("attention.2.bias", "attention_c.bias")


def _same(got, want, key, tol, scale=None):
    """Bit for bit, up to the order of float atomics (module docstring): ``tol`` of ``scale``, the largest entry of ``want`` by
    default."""
    if got is None or want is None:
        assert got is None and want is None, key
        return
    assert got.shape == want.shape and got.dtype == want.dtype, key
    if torch.equal(got, want):
        return
    d = (got.float() - want.float()).abs().max().item()
    assert d <= tol * (want.float().abs().max().item() if scale is None else scale), (key, d)


def _top(grads):
    return max(g.abs().max().item() for g in grads.values() if g is not None)


def _same_all(got, want, tag, tol):
    """Parameter gradients.  The score layer's bias has a zero gradient in exact arithmetic (a soft-max shift): only rounding
    noise, bounded by the largest gradient of the module."""
    assert got.keys() == want.keys()
    for k in want:
        _same(got[k], want[k], f"{tag}: {k}", tol, _top(want) if k.endswith(SHIFT_BIASES) else None)


def _fresh(case):
    m = case.build()
    inp = case.inputs()
    return m, inp


def _forward(case, m, inp, wrap=None):
    torch.manual_seed(case.seed)                       # the dropout draws of the forward (and of nothing else)
    if wrap is None:
        return case.fwd(m, inp)
    return wrap(lambda: case.fwd(m, inp))


@functools.lru_cache(maxsize=None)
def _route1(name):
    """Plain backward: (output, parameter gradients, input gradient)."""
    case = CASES[name]
    m, inp = _fresh(case)
    loss, out = _forward(case, m, inp)
    loss.backward()
    xin = case.xin(inp)
    return out.detach().clone(), _grads(m), xin.grad.detach().clone()


def _frag_views_in_use(case):
    from murcl_amd import functional, ops
    m = case.build()
    e, a = m.encoder, m.attention
    assert functional.abmil_fast_path(4 * 2048, 2048, 512, 512, 128, BF16) and functional._FRAG_WEIGHTS
    views = ops.weight_views(functional._frag_specs(e[0].weight, e[3].weight, e[6].weight, a[0].weight, BF16))
    assert [ops.is_frag(v) for v in views] == [True, True, True, True, False, True, True]


# ---------------------------------------------------------------- route 1: the anchor
@pytest.mark.parametrize("name", NAMES)
def test_plain_backward_vs_oracle(name):
    case = CASES[name]
    if name in ("abmil_bf16", "abmil_dropout_bf16"):
        _frag_views_in_use(case)
    out, grads, gx = _route1(name)
    assert any(v is not None for v in grads.values())
    case.oracle(case, out, grads, gx)


# ---------------------------------------------------------------- route 2: saved-tensor hooks that copy
HOOKS = {
    "save_on_cpu": lambda: torch.autograd.graph.save_on_cpu(pin_memory=False),
    "save_on_cpu_pinned": lambda: torch.autograd.graph.save_on_cpu(pin_memory=True),
    "clone": lambda: torch.autograd.graph.saved_tensors_hooks(lambda t: t.clone(), lambda t: t),
}


@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("name", NAMES)
def test_saved_tensor_hooks_give_the_plain_gradients(name, hook):
    case = CASES[name]
    out1, g1, gx1 = _route1(name)
    m, inp = _fresh(case)
    with HOOKS[hook]():
        loss, out = _forward(case, m, inp)
    loss.backward()
    tol = _tol(name)
    _same(out.detach(), out1, "out", tol)
    _same(case.xin(inp).grad, gx1, "input", tol)
    _same_all(_grads(m), g1, hook, tol)


# ---------------------------------------------------------------- route 3: activation checkpointing
@pytest.mark.parametrize("name", NAMES)
def test_checkpoint_gives_the_plain_gradients(name):
    """The recomputation inside backward runs the forward again; with training-mode Dropout it must draw the masks the first
    forward drew (route 1 ran after the same ``torch.manual_seed``: the reference draws the same masks, not checkpointed)."""
    from torch.utils.checkpoint import checkpoint
    case = CASES[name]
    out1, g1, gx1 = _route1(name)
    m, inp = _fresh(case)
    loss, out = _forward(case, m, inp, wrap=lambda f: checkpoint(f, use_reentrant=False))
    loss.backward()
    tol = _tol(name)
    _same(out.detach(), out1, "out", tol)
    _same(case.xin(inp).grad, gx1, "input", tol)
    _same_all(_grads(m), g1, "checkpoint", tol)


def test_dropout_draws_differ_between_calls_but_replay_under_a_seed():
    """What route 3 relies on, stated on its own: the training-mode masks are torch RNG draws (two calls, two masks; the same
    seed, the same masks) - so the checkpoint test above compares against the masks actually drawn."""
    case = CASES["abmil_dropout_f32"]
    m, inp = _fresh(case)
    with torch.no_grad():
        a = _forward(case, m, inp)[1].clone()
        b = case.fwd(m, inp)[1].clone()
        c = _forward(case, m, inp)[1].clone()
    assert not torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------- route 4: partial backward with direct accumulation on
@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_partial_backward_leaves_the_seated_gradients_alone(name, deferred, monkeypatch):
    import contextlib
    from murcl_amd import functional
    from murcl_amd.optim import FlatAdam
    case = CASES[name]
    out1, g1, gx1 = _route1(name)
    monkeypatch.setattr(functional, "_DIRECT", functional._DIRECT)        # (FlatAdam switches it on for the process: restored after)
    m, inp = _fresh(case)
    params = dict(m.named_parameters())
    FlatAdam([{"params": list(params.values()), "lr": 1e-4}], betas=(0.9, 0.999), weight_decay=1e-5)
    assert functional._DIRECT and all(p.grad is not None for p in params.values())
    touched = []
    real_touch = functional._touch
    monkeypatch.setattr(functional, "_touch", lambda *ps: (touched.extend(p for p in ps if p is not None), real_touch(*ps))[1])
    snap = _grads(m)
    xin = case.xin(inp)
    tol = _tol(name)
    scope = functional.deferred_wgrads if deferred else contextlib.nullcontext

    # backward(inputs=[x]): x.grad as plain backward's, no p.grad changes
    with scope():
        loss, _ = _forward(case, m, inp)
        loss.backward(inputs=[xin])
    _same(xin.grad, gx1, "backward(inputs=[x]) input", tol)
    _same_all(_grads(m), snap, "backward(inputs=[x]) leaves .grad", 0.0)
    # autograd.grad(loss, [x])
    with scope():
        loss, _ = _forward(case, m, inp)
        gx, = torch.autograd.grad(loss, [xin])
    _same(gx, gx1, "grad(loss, [x])", tol)
    _same_all(_grads(m), snap, "grad(loss, [x]) leaves .grad", 0.0)
    # autograd.grad(loss, params): plain backward's gradients returned, none accumulated
    with scope():
        loss, _ = _forward(case, m, inp)
        gp = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
    _same_all({k: g for k, g in zip(params, gp)}, g1, "grad(loss, params)", tol)
    _same_all(_grads(m), snap, "grad(loss, params) leaves .grad", 0.0)
    assert not touched
    # plain backward in the same process still accumulates straight into the flat buffer
    with scope():
        loss, _ = _forward(case, m, inp)
        loss.backward()
    got = _grads(m)
    top = _top(g1)
    for k in g1:
        if g1[k] is None:
            assert not got[k].any(), k                         # (never reached: the seated zeros stay)
            continue
        scale = top if k.endswith(SHIFT_BIASES) else g1[k].abs().max().item()        # (as in _same_all)
        d = (got[k] - g1[k]).abs().max().item()
        assert d <= max(1e-5, tol) * scale, (k, d)
    if case.direct:
        assert touched and {id(p) for p in touched} <= {id(p) for p in params.values()}
    else:
        assert not touched


# ---------------------------------------------------------------- route 5: forward only
@pytest.mark.parametrize("mode", ["no_grad", "inference_mode"])
@pytest.mark.parametrize("name", NAMES)
def test_forward_only_calls_give_the_training_forward(name, mode):
    """Forward-only calls take their own kernels in places (no ReLU masks written, CLAM's gate score from the gate GEMM's epilogue):
    the f32 paths agree with the training forward to 1e-5 of the largest entry, the bf16 paths to their storage precision."""
    case = CASES[name]
    out1 = _route1(name)[0]
    m, inp = _fresh(case)
    ctx = torch.no_grad() if mode == "no_grad" else torch.inference_mode()
    with ctx:
        loss, out = _forward(case, m, inp)
    assert not out.requires_grad
    tol = 2e-3 if out1.dtype == BF16 or "bf16" in name else 1e-5
    d = (out.float() - out1.float()).abs().max().item()
    assert d <= tol * out1.float().abs().max().item(), d
