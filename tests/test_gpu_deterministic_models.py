"""Deterministic mode through the models and the training steps: in the mode ``murcl_float_atomic_launches()`` stays put over
forward + backward (resp. over whole training steps) and two runs from the same inputs / the same seed and initial parameters give
bit-identical outputs, parameter gradients, parameters and Adam moments.  Each thing runs twice, not in a loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import murcl_amd  # noqa: E402
from murcl_amd import functional, ops  # noqa: E402
from oracle import detrand, params as P  # noqa: E402

T = torch.from_numpy


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _tensors(res):
    if torch.is_tensor(res):
        return [res] if res.is_floating_point() else []
    if isinstance(res, dict):
        res = list(res.values())
    if isinstance(res, (list, tuple)):
        return [t for r in res for t in _tensors(r)]
    return []


def _forward_backward(model, call):
    """-> ([outputs], {parameter: gradient}) of one forward + backward; the loss is the sum of squares of every differentiable output."""
    model.zero_grad(set_to_none=True)
    outs = _tensors(call())
    loss = sum(o.float().square().sum() for o in outs if o.requires_grad)
    loss.backward()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs], {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _check_model(model, call, min_grads):
    with murcl_amd.deterministic():
        c0 = ops.float_atomic_launches()
        o1, g1 = _forward_backward(model, call)
        o2, g2 = _forward_backward(model, call)
        assert ops.float_atomic_launches() == c0, "an arrival-order form was launched in deterministic mode"
    assert not murcl_amd.is_deterministic()
    assert len(o1) == len(o2) and len(o1) > 0 and sorted(g1) == sorted(g2) and len(g1) >= min_grads
    for a, b in zip(o1, o2):
        assert torch.isfinite(a).all() and torch.equal(a, b), "outputs differ between two calls"
    for k in g1:
        assert torch.isfinite(g1[k]).all() and torch.equal(g1[k], g2[k]), f"gradient of {k} differs between two calls"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32-generic", "bf16-fast"])
def test_abmil(dtype):
    from murcl_amd.models.abmil import ABMIL
    m = ABMIL(512, L=512, D=128, dim_out=128)
    m.load_state_dict(P.to_torch(P.abmil(41)))
    m.compute_dtype = dtype
    m = m.to(_dev())
    x = T(P.bags(41, "x", 2, 256, 512)).to(_dev())
    _check_model(m, lambda: m(x), min_grads=8)


def test_clam_sb_eval_with_instance_loss():
    from murcl_amd.models.clam import CLAM_SB
    m = CLAM_SB(gate=True, size_arg="small", dropout=True, k_sample=8, n_classes=2, subtyping=True, in_dim=512)
    m.load_state_dict(P.to_torch(P.clam_sb(42)))
    m = m.to(_dev()).eval()
    x = T(P.bags(42, "x", 2, 512, 512)).to(_dev())

    def call():
        M, _, res = m(x, label=[1, 0], instance_eval=True)
        return [M] + [r["instance_loss"] for r in res]

    # by default the pooled vector M = A h is a weighted_rowsum whose row splits meet through atomics: the shape reaches such a form
    c0 = ops.float_atomic_launches()
    _forward_backward(m, call)
    assert ops.float_atomic_launches() > c0
    _check_model(m, call, min_grads=8)


def _dsmil(d, C, dropout_v=0.0):
    from murcl_amd.models.dsmil import BClassifier, FCLayer, MILNet
    m = MILNet(FCLayer(d, C), BClassifier(d, C, dropout_v=dropout_v))
    m.load_state_dict(P.to_torch(P.dsmil(43, d, C)))
    return m.to(_dev())


@pytest.mark.parametrize("route", ["stream", "explicit", "literal"])
def test_dsmil(route):
    B, N, d = 2, 512, 64
    C = 5 if route == "literal" else 2
    dev = _dev()
    m = _dsmil(d, C, dropout_v=0.25 if route == "explicit" else 0.0)
    x = T(P.bags(43, f"x{route}", B, N, d)).to(dev)
    want = {"stream": (True, True, True), "explicit": (True, True, False), "literal": (False, False, False)}[route]
    assert tuple(functional.dsmil_route(B, N, d, C, route == "explicit")) == want
    if route == "explicit":
        m = m.train()
        keep = ((detrand.uniform(43, "keep", (B, N, d)) >= 0.25).astype(np.float32) / np.float32(0.75)).astype(np.float32)
        m.keep_mask_v = T(keep).to(dev)
    else:
        m = m.eval()

    def call():
        classes, bag, _ = m(x)
        return [torch.stack(classes), bag]

    if route != "stream":           # (the one-pass kernels of the stream route leave per-wave partial rows: no atomics by default either)
        c0 = ops.float_atomic_launches()
        _forward_backward(m, call)
        assert ops.float_atomic_launches() > c0
    _check_model(m, call, min_grads=4)


# ------------------------------------------------------------------ training steps
def _args(**kw):
    from murcl_amd.train_MuRCL import build_parser
    a = build_parser().parse_args(["--arch", "ABMIL"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _state(modules, opts):
    out = {}
    for i, mod in enumerate(modules):
        out.update({f"{i}.{k}": v.detach().clone() for k, v in mod.state_dict().items()})
    for i, opt in enumerate(opts):
        for j, g in enumerate(opt.state_dict(on_device=True)["groups"]):
            out.update({f"opt{i}.{j}.{name}": g[name] for name in ("m", "v")})
    torch.cuda.synchronize()
    return out


def _same_state(a, b):
    assert sorted(a) == sorted(b) and len(a) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs from the same seed ({int((a[k] != b[k]).sum())}/{a[k].numel()} elements)"


@pytest.mark.parametrize("stage", [1, 2])
def test_three_pretrain_steps_twice(stage, tmp_path):
    from murcl_amd.models import rlmil
    from murcl_amd.train_MuRCL import create_model, get_optimizer, pretrain_step
    from murcl_amd.utils.datasets import BagPack
    from murcl_amd.utils.losses import NT_Xent
    dev = _dev()
    B, N, K, fs, Tn = 4, 600, 10, 128, 2
    feats = [T(P.bags(44, f"f{b}", 1, N + 13 * b, 512)[0]).to(dev) for b in range(B)]
    pack = BagPack.from_lists(feats, [P.cluster_lists(44, f"c{b}", N + 13 * b, K) for b in range(B)])
    torch.manual_seed(5)
    a1 = _args(T=Tn, feat_size=fs, batch_size=B, dtype="f32", train_stage=1, num_clusters=K, backbone_lr=1e-3, fc_lr=1e-3,
               save_dir=str(tmp_path / "stage_1"))
    m1, f1, _ = create_model(a1, 512, dev)
    (tmp_path / "stage_1").mkdir()
    torch.save({"model_state_dict": m1.state_dict(), "fc": f1.state_dict()}, tmp_path / "stage_1" / "model_best.pth.tar")
    args = a1 if stage == 1 else _args(T=Tn, feat_size=fs, batch_size=B, dtype="f32", train_stage=2, num_clusters=K, K_epochs=2,
                                       save_dir=str(tmp_path / "stage_2"), ppo_lr=1e-3)

    def run():
        torch.manual_seed(6)                                         # the same initial parameters (stage 2: the policy's) and the same draws
        model, fc, ppo = create_model(args, 512, dev)
        if stage == 1:
            model.load_state_dict(m1.state_dict())
            fc.load_state_dict(f1.state_dict())
        opt = get_optimizer(args, model, fc)
        assert (opt is None) == (stage == 2)
        before = _state([model, fc] + ([ppo.policy] if ppo else []), [])
        for _ in range(3):
            loss, _, _ = pretrain_step(args, model, fc, ppo, NT_Xent(B, 1.0), opt, pack, [rlmil.Memory(), rlmil.Memory()])
            assert torch.isfinite(loss)
        opts = [opt] if opt is not None else [ppo.optimizer]
        return before, _state([model, fc] + ([ppo.policy, ppo.policy_old] if ppo else []), opts)

    with murcl_amd.deterministic():
        c0 = ops.float_atomic_launches()
        b1, s1 = run()
        b2, s2 = run()
        assert ops.float_atomic_launches() == c0, "an arrival-order form was launched in deterministic mode"
    _same_state(b1, b2)
    _same_state(s1, s2)
    moved = [k for k in b1 if k.startswith("0." if stage == 1 else "2.") and k.endswith("weight") and not torch.equal(s1[k], b1[k])]
    assert moved, "the steps trained nothing"          # stage 1: the encoder; stage 2: the policy (PPO update)


@pytest.mark.parametrize("arch", ["ABMIL", "CLAM_SB", "DSMIL"])
def test_supervised_step_twice(arch):
    from murcl_amd.models import rlmil
    from murcl_amd.optim import FlatAdam
    from murcl_amd.train_RLMIL import create_model, supervised_step
    from murcl_amd.utils.datasets import BagPack
    dev = _dev()
    B, N, K, fs, C = 4, 500, 10, 128, 2
    pk = P.abmil(61, dim_out=C) if arch == "ABMIL" else {"CLAM_SB": P.clam_sb, "DSMIL": P.dsmil}[arch](61)
    fcp = P.full_layer(61, 512, 1024, C)
    pack = BagPack.from_lists([T(P.bags(61, f"f{b}", 1, N, 512)[0]).to(dev) for b in range(B)], [P.cluster_lists(61, f"c{b}", N, K) for b in range(B)])
    labels = torch.tensor([0, 1, 1, 0], device=dev)
    acts = [T(detrand.uniform(61, f"a{t}", (B, K))) for t in range(2)]

    def run():
        torch.manual_seed(7)
        model, fc = create_model(arch, 512, C, dev)
        model.load_state_dict(P.to_torch(pk))
        fc.load_state_dict(P.to_torch(fcp))
        opt = FlatAdam([{"params": list(model.parameters()) + list(fc.parameters()), "lr": 1e-3}])
        loss, _, _ = supervised_step(arch, model, fc, None, opt, pack, labels, rlmil.Memory(), T=2, feat_size=fs, actions=acts)
        assert torch.isfinite(loss)
        return _state([model, fc], [opt]), loss.detach().clone()

    with murcl_amd.deterministic():
        c0 = ops.float_atomic_launches()
        (s1, l1), (s2, l2) = run(), run()
        assert ops.float_atomic_launches() == c0, "an arrival-order form was launched in deterministic mode"
    _same_state(s1, s2)
    assert torch.equal(l1, l2)
    assert not torch.equal(s1["1.fc.weight"], P.to_torch(fcp)["fc.weight"].to(dev)), "the step trained nothing"
