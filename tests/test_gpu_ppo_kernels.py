"""The sampler's native launch sequences (csrc/ppo_seq.hip) and the per-launch head kernels (csrc/ppo.hip) against a plain
float64 reference: oracle/mil_oracle.py's ``ppo_act`` / ``ppo_evaluate`` / ``ppo_loss`` fed ``.double()`` tensors, gradients by
autograd.

The inputs put rows on every branch of the clipped surrogate: ratio ~ 1.65, 0.61, 1.05, 0.95 and 1 crossed with advantages of
both signs, each row at least 0.1 away from the clip edges and with |adv| >= 0.25, so no f32 / f64 branch flip can occur and a
kernel that ignores or misroutes the clip misses the bound by a wide margin (the preconditions below assert all of that on the
float64 reference alone, before the GPU is touched).

These are f32 kernels: per tensor |got - ref| <= 1e-4 * max|ref| + 1e-4 * |ref| (BASELINE.json north_star).

Not covered: the unfused GRU branch of ``ps_epoch`` / ``murcl_ppo_act`` - every H the sequences admit (H % 32 == 0) is also
a shape ``murcl_gru_step_supported`` accepts, so that branch cannot be reached through the C interface."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detrand, mil_oracle as O, params as P  # noqa: E402

T = torch.from_numpy
STD, EPS_CLIP, SEED = 0.5, 0.2, 71
DELTA = (0.5, -0.5, 0.05, -0.05, 0.0)          # log-ratio classes by row % 5: ratio ~ 1.65, 0.61, 1.05, 0.95, 1
EPOCH_CASES = [(64, 32, 1, 1, 5), (32, 96, 16, 2, 20), (64, 32, 3, 3, 11), (96, 64, 10, 1, 33), (512, 512, 10, 4, 12)]
ACT_CASES = [(64, 32, 1, 1), (32, 96, 16, 5), (512, 512, 10, 33)]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _close(got, want, rtol, atol, msg=""):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    bad = err > tol
    assert not bad.any(), f"{msg}: {int(bad.sum())}/{bad.numel()} off, max err {err.max():.3e} (ref max {want.abs().max():.3e})"


def _contract(got, ref, msg, base=None):
    """The f32 contract on one tensor.  ``base``: the f32 values the kernel added its result to; they are taken off again in
    float64 (exact up to the one f32 rounding of the kernel's add), so the bound comes from ``ref`` alone."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.detach().double()
    if base is not None:
        got = got - base.double()
    top = ref.abs().max().item()
    print(f"{msg}: max err {(got - ref).abs().max().item():.3e}, max |ref| {top:.3e}")
    _close(got, ref, rtol=1e-4, atol=1e-4 * top, msg=msg)


# ------------------------------------------------------------------ inputs and the float64 reference (host only)
@functools.lru_cache(maxsize=None)
def _inputs(S, H, K, Tn, B, seed=SEED):
    """f32 inputs of one epoch and their float64 copies: the reference reads exactly the bits the kernels read."""
    p32 = P.to_torch(P.actor_critic(seed, S, H, K))
    p64 = {k: v.double() for k, v in p32.items()}
    states = T(detrand.normal(seed, "s", (Tn, B, S)))
    eps = T(detrand.normal(seed, "e", (Tn, B, K))).double()
    with torch.no_grad():
        h, acts = torch.zeros(B, H, dtype=torch.float64), []
        for t in range(Tn):                                     # a float64 rollout: ~15 % of the actions clamped at 0, ~15 % at 1
            a, _, h = O.ppo_act(p64, states[t].double(), h, eps[t], STD)
            acts.append(a)
        actions = torch.stack(acts, 0).float()
        lp0, v0 = O.ppo_evaluate(p64, states.double(), actions.double(), STD)[:2]
    row = torch.arange(Tn * B).view(Tn, B)
    delta = torch.tensor(DELTA, dtype=torch.float64)[row % 5]
    sign = torch.where((row // 5) % 2 == 0, 1.0, -1.0).double()
    mag = T(detrand.uniform(seed, "m", (Tn, B), 0.3, 1.5)).double()
    old_logp = (lp0 - delta).float()
    returns = (v0 + sign * mag).float()
    return dict(p32=p32, p64=p64, states=states, actions=actions, old_logp=old_logp, returns=returns)


def _rows(p, inp, eps_clip):
    """Per-row terms of PPO.update's loss in float64 (rlmil.py:169-178)."""
    logp, value, ent = O.ppo_evaluate(p, inp["states"].double(), inp["actions"].double(), STD)
    ret = inp["returns"].double()
    ratio = torch.exp(logp - inp["old_logp"].double())
    adv = ret - value.detach()
    s1, s2 = ratio * adv, ratio.clamp(1 - eps_clip, 1 + eps_clip) * adv
    return ratio, adv, -torch.min(s1, s2) + 0.5 * (value - ret) ** 2 - 0.01 * ent


@functools.lru_cache(maxsize=None)
def _reference(case, n_mult, eps_clip=EPS_CLIP):
    """(loss, {name: gradient}) of sum_rows(-min(s1, s2) + 0.5 (v - R)^2 - 0.01 ent) / n_total in float64, n_total = n_mult * R."""
    inp = _inputs(*case)
    p = {k: v.clone().requires_grad_() for k, v in inp["p64"].items()}
    n_total = n_mult * case[3] * case[4]
    loss = _rows(p, inp, eps_clip)[2].sum() / n_total
    loss.backward()
    if n_mult == 1:                                             # the hand-written form is the oracle's own loss
        with torch.no_grad():
            ref = O.ppo_loss(inp["p64"], inp["states"].double(), inp["actions"].double(), inp["old_logp"].double(),
                             inp["returns"].double(), STD, eps_clip)
        assert abs(loss.item() - ref.item()) <= 1e-12, (loss.item(), ref.item())
    return loss.detach(), {k: v.grad for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def _precondition_figures(case):
    inp = _inputs(*case)
    with torch.no_grad():
        ratio, adv, _ = _rows(inp["p64"], inp, EPS_CLIP)
    ratio, adv = ratio.flatten(), adv.flatten()
    margin = torch.minimum((ratio - (1 - EPS_CLIP)).abs(), (ratio - (1 + EPS_CLIP)).abs()).min().item()
    hi, lo = ratio > 1 + EPS_CLIP, ratio < 1 - EPS_CLIP
    classes = [int((hi & (adv > 0)).sum()), int((hi & (adv < 0)).sum()), int((lo & (adv > 0)).sum()), int((lo & (adv < 0)).sum()),
               int((~hi & ~lo).sum())]
    g, g10 = _reference(case, 1)[1]["actor.0.weight"], _reference(case, 1, 10.0)[1]["actor.0.weight"]
    return margin, adv.abs().min().item(), classes, ((g - g10).norm() / g.norm()).item()


def _preconditions(case):
    """Conditions on the inputs, on the float64 reference alone: every test calls this before it touches the GPU."""
    margin, min_adv, classes, clip_diff = _precondition_figures(case)
    assert margin >= 0.1, f"a ratio sits {margin:.3f} from a clip edge"
    assert min_adv >= 0.25, f"min |adv| {min_adv:.3f}"
    if case[3] * case[4] >= 20:
        assert min(classes) >= 1, f"rows per clip class {classes}"
    assert clip_diff > 0.10, f"the clip changes d(actor.0.weight) by only {clip_diff:.3f}"
    return margin, min_adv, classes, clip_diff


def _policy(case, dev):
    from murcl_amd.models.rlmil import ActorCritic
    S, H, K = case[:3]
    pol = ActorCritic(S, S, H, False, action_std=STD, action_size=K)
    pol.load_state_dict(_inputs(*case)["p32"])
    return pol.to(dev)


def _run_epoch(case, dev, n_mult, given_wt, want_loss=True):
    """ops.ppo_epoch on a fresh policy whose gradient tensors hold a seeded non-zero g0 -> (loss, {name: gradient}, {name: g0})."""
    from murcl_amd import ops
    S, H, K, Tn, B = case
    inp, grads = _inputs(*case), _reference(case, n_mult)[1]
    pol = _policy(case, dev)
    assert pol._native_ok(S)
    g0 = {}
    for name, p in pol.named_parameters():
        top = grads[name].abs().max().item()                    # (0 for W_hh at T = 1: that buffer must come back untouched)
        g0[name] = T(detrand.normal(SEED, "g0." + name, tuple(p.shape))) * np.float32(0.5 * top if top > 0 else 1.0)
        p.grad = g0[name].to(dev)
    wt = None
    if given_wt:
        wt = [w.detach().t().contiguous() for w in (pol.gru.weight_ih_l0, pol.gru.weight_hh_l0, pol.state_encoder[2].weight)]
    loss = ops.ppo_epoch(pol.pointer_table(), pol.pointer_table(grads=True), S, H, K, inp["states"].to(dev), inp["actions"].to(dev),
                         inp["old_logp"].to(dev), inp["returns"].to(dev), n_mult * Tn * B, STD, EPS_CLIP, O.gaussian_entropy(K, STD),
                         want_loss=want_loss, wt=wt)
    torch.cuda.synchronize()
    return loss, {name: p.grad.detach().cpu() for name, p in pol.named_parameters()}, g0


# ------------------------------------------------------------------ 1. murcl_ppo_epoch / murcl_ppo_epoch_wt
@pytest.mark.parametrize("n_mult", [1, 3])
@pytest.mark.parametrize("given_wt", [False, True])
@pytest.mark.parametrize("case", EPOCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_ppo_epoch_against_float64(case, given_wt, n_mult):
    """One native K_epoch: the loss and all 12 parameter gradients, ADDED into non-zero buffers, with the transposes made by the
    call (``murcl_ppo_epoch``) or handed in (``murcl_ppo_epoch_wt``), alone (n_total = R) or as one of three ranks (3R)."""
    _preconditions(case)
    ref_loss, ref_grads = _reference(case, n_mult)
    loss, grads, g0 = _run_epoch(case, _dev(), n_mult, given_wt)
    _contract(loss, ref_loss.reshape(1), "loss")
    assert len(grads) == 12
    for name, ref in ref_grads.items():
        assert ref.abs().max().item() > 0 or (name == "gru.weight_hh_l0" and case[3] == 1), name
        _contract(grads[name], ref, name, base=g0[name])


def test_ppo_epoch_without_loss_out_gives_the_same_bits():
    """``loss_out`` = NULL (what PPO.update passes) changes nothing else: the gradients equal the ``want_loss`` run bit for bit."""
    case = EPOCH_CASES[1]
    _preconditions(case)
    dev = _dev()
    loss, with_loss, _ = _run_epoch(case, dev, 1, False, want_loss=True)
    none, without, _ = _run_epoch(case, dev, 1, False, want_loss=False)
    assert loss is not None and none is None
    for name in with_loss:
        assert torch.equal(with_loss[name], without[name]), name


# ------------------------------------------------------------------ 2. murcl_ppo_act
@pytest.mark.parametrize("with_hidden", [False, True])
@pytest.mark.parametrize("S,H,K,B", ACT_CASES)
def test_ppo_act_against_float64(S, H, K, B, with_hidden):
    """One native sampling step from the zero state (hidden_prev = NULL) and from a given one: hidden state, action, log-prob;
    actions the reference clamps by more than 1e-3 are exactly 0.0 / 1.0."""
    from murcl_amd import ops
    p32 = P.to_torch(P.actor_critic(SEED, S, H, K))
    p64 = {k: v.double() for k, v in p32.items()}
    state, eps = T(detrand.normal(SEED, "s", (B, S))), T(detrand.normal(SEED, "e", (B, K)))
    hid = T(detrand.normal(SEED, "h", (B, H)) * np.float32(0.5)) if with_hidden else None
    with torch.no_grad():
        h0 = hid.double() if with_hidden else torch.zeros(B, H, dtype=torch.float64)
        a_ref, lp_ref, h_ref = O.ppo_act(p64, state.double(), h0, eps.double(), STD)
        raw = torch.sigmoid(h_ref @ p64["actor.0.weight"].t() + p64["actor.0.bias"]) + STD * eps.double()
    below, above = raw < -1e-3, raw > 1 + 1e-3
    if B * K >= 30:
        assert below.any() and above.any() and ((raw > 1e-3) & (raw < 1 - 1e-3)).any()
    dev = _dev()
    from murcl_amd.models.rlmil import ActorCritic
    pol = ActorCritic(S, S, H, False, action_std=STD, action_size=K)
    pol.load_state_dict(p32)
    pol = pol.to(dev)
    assert pol._native_ok(S)
    h, a, lp = ops.ppo_act(pol.pointer_table(), S, H, K, state.to(dev), hid.to(dev) if with_hidden else None, eps.to(dev), STD)
    _contract(h, h_ref, "hidden_new")
    _contract(a, a_ref, "action")
    _contract(lp, lp_ref, "logp")
    a = a.cpu()
    assert (a[below] == 0.0).all() and (a[above] == 1.0).all()
    assert a.min().item() >= 0.0 and a.max().item() <= 1.0


# ------------------------------------------------------------------ 3. the per-launch autograd path on the same inputs
@pytest.mark.parametrize("n_mult", [1, 3])
@pytest.mark.parametrize("case", [EPOCH_CASES[2], EPOCH_CASES[4]], ids=lambda c: "x".join(map(str, c)))
def test_fallback_epoch_against_float64(case, n_mult):
    """``_HipPolicyKernels.epoch_grads`` with the native sequences switched off: ActorCritic.evaluate (LinearFn, GRUSeqFn,
    PolicyHeadFn) + PPOLossFn on clipped rows, alone and as one of three ranks, against the same float64 reference."""
    from murcl_amd.models.rlmil import PPO, _HipPolicyKernels
    _preconditions(case)
    S, H, K, Tn, B = case
    inp, ref_grads = _inputs(*case), _reference(case, n_mult)[1]
    dev = _dev()
    ppo = PPO(S, S, H, False, action_std=STD, lr=1e-4, gamma=0.1, K_epochs=1, eps_clip=EPS_CLIP, action_size=K)
    ppo.policy.load_state_dict(inp["p32"])
    ppo.policy._native_ok = lambda S_: False
    _HipPolicyKernels.epoch_grads(ppo, inp["states"].to(dev), inp["actions"].to(dev), inp["old_logp"].to(dev), inp["returns"].to(dev),
                                  n_mult * Tn * B)
    torch.cuda.synchronize()
    grads = dict(ppo.policy.named_parameters())
    assert len(grads) == 12
    for name, ref in ref_grads.items():
        _contract(grads[name].grad, ref, name)


# ------------------------------------------------------------------ 4. murcl_policy_head_fwd / murcl_policy_head_bwd
@pytest.mark.parametrize("K", [1, 10, 64])
@pytest.mark.parametrize("R", [1, 257])
def test_policy_head_fwd_bwd_against_float64(R, K):
    """Both modes of the forward kernel (sample with eps; evaluate given actions) and the backward kernel; R = 257 is two
    workgroups with a one-row tail."""
    from murcl_amd import ops
    z = T(detrand.normal(SEED, "z", (R, K)) * np.float32(2.0))
    eps = T(detrand.normal(SEED, "e", (R, K)))
    acts = T(detrand.uniform(SEED, "a", (R, K), -0.2, 1.2)).clamp(0.0, 1.0)         # given actions: some exactly 0.0 and 1.0
    dlogp = T(detrand.normal(SEED, "d", (R,)))
    z64 = z.double().requires_grad_()
    mu_ref = torch.sigmoid(z64)
    raw = mu_ref.detach() + STD * eps.double()
    a_ref = raw.clamp(0.0, 1.0)
    lp_sample = O.gaussian_logprob(a_ref, mu_ref.detach(), STD)
    lp_eval = O.gaussian_logprob(acts.double(), mu_ref, STD)
    (lp_eval * dlogp.double()).sum().backward()
    dev = _dev()
    mu, a, lp = ops.policy_head_fwd(z.to(dev), STD, eps=eps.to(dev))
    _contract(mu, mu_ref, "mu (sample)")
    _contract(a, a_ref, "action")
    _contract(lp, lp_sample, "logp (sample)")
    a = a.cpu()
    assert (a[raw < -1e-3] == 0.0).all() and (a[raw > 1 + 1e-3] == 1.0).all()
    mu, a, lp = ops.policy_head_fwd(z.to(dev), STD, actions=acts.to(dev))
    assert torch.equal(a.cpu(), acts)
    _contract(mu, mu_ref, "mu (evaluate)")
    _contract(lp, lp_eval, "logp (evaluate)")
    dz = ops.policy_head_bwd(mu, a, dlogp.to(dev), STD)
    _contract(dz, z64.grad, "dz")
