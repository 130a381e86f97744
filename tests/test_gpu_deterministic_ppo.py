"""Deterministic mode through the native PPO epoch (murcl_ppo_epoch / murcl_ppo_epoch_wt) on a rollout of more than 512 rows - what
the entry script's defaults give (T = 6 patch steps x 128 bags = 768 rows).  Its weight gradients plan as ATOMIC by default and the
column sums of dgh split their rows; in the mode they plan as PARTS resp. take murcl_colsum_det's form, with the workspace carved
out of the epoch's own (murcl_ppo_epoch_workspace).  Inputs, float64 reference and bound are tests/test_gpu_ppo_kernels.py's."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import murcl_amd  # noqa: E402
from murcl_amd import ops  # noqa: E402
from tests import test_gpu_ppo_kernels as PK  # noqa: E402

CASE = (32, 32, 3, 3, 200)                     # (S, H, K, T, B): 600 rows, the last weight gradient over 400


@pytest.mark.parametrize("given_wt", [False, True])
def test_ppo_epoch_beyond_512_rows(given_wt):
    dev = PK._dev()
    ref_loss, ref_grads = PK._reference(CASE, 1)
    assert not murcl_amd.is_deterministic()
    c0 = ops.float_atomic_launches()
    loss_d, grads_d, g0 = PK._run_epoch(CASE, dev, 1, given_wt)
    assert ops.float_atomic_launches() > c0, "this rollout does not reach an arrival-order form in default mode: wrong shape"
    with murcl_amd.deterministic():
        c1 = ops.float_atomic_launches()
        loss1, grads1, _ = PK._run_epoch(CASE, dev, 1, given_wt)
        loss2, grads2, _ = PK._run_epoch(CASE, dev, 1, given_wt)
        assert ops.float_atomic_launches() == c1, "an arrival-order form was launched in deterministic mode"
    assert torch.equal(loss1, loss2) and sorted(grads1) == sorted(grads2) and len(grads1) == 12
    for name in grads1:
        assert torch.equal(grads1[name], grads2[name]), f"{name} differs between two epochs in deterministic mode"
    for tag, loss, grads in (("in the mode", loss1, grads1), ("by default", loss_d, grads_d)):
        PK._contract(loss, ref_loss.reshape(1), f"loss {tag}")
        for name, ref in ref_grads.items():
            PK._contract(grads[name], ref, f"{name} {tag}", base=g0[name])


def test_ppo_update_with_the_entry_script_defaults_runs_in_the_mode():
    """PPO.update over T = 6 x 128 bags (768 rows, --T / --batch_size defaults): twice from the same policy, same bits."""
    from murcl_amd.models import rlmil
    dev = PK._dev()
    Tn, B, S = 6, 128, 64
    g = torch.Generator().manual_seed(3)
    states = [torch.randn((B, S), generator=g).to(dev) for _ in range(Tn)]
    rewards = [torch.rand((1, B), generator=g).to(dev) for _ in range(Tn)]

    def run():
        torch.manual_seed(11)
        ppo = rlmil.PPO(S, S, 32, False, action_std=0.5, lr=1e-3, K_epochs=2, action_size=3)
        mem = rlmil.Memory()
        for t in range(Tn):
            ppo.select_action(states[t], mem, restart_batch=(t == 0))
        mem.rewards.extend(rewards)
        ppo.update(mem)
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in ppo.policy.state_dict().items()}

    with murcl_amd.deterministic():
        c0 = ops.float_atomic_launches()
        a, b = run(), run()
        assert ops.float_atomic_launches() == c0
    assert all(torch.isfinite(v).all() and torch.equal(v, b[k]) for k, v in a.items())
