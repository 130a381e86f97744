"""Cost of deterministic mode (murcl_amd.set_deterministic) against default mode on the same tree, in ONE process: the C2 bf16
pre-training step (64 bags x 2 views x 2048 x 512), CLAM-SB C3 forward + backward with instance loss (64 x 4096 x 512 bf16) and
the DSMIL C5 share (16 x 8192 x 1024 f32) - the workloads of bench.py, built by bench.py's own helpers.  The two modes alternate
(default, mode, default, mode ...), `--rounds` windows each of `--reps` back-to-back passes between one pair of events; per
workload and mode it prints the median window (ms per pass), the spread (min .. max) and the arrival-order launches per pass.
Also times, in both modes, the sites the three workloads do not reach: the bag-level gemm_nt that splits K by default
([33 x 40 x 1536] f32), bag-level weight gradients that are ATOMIC / WIDE by default, and one native PPO epoch over 768 rows.

    python tools/det_cost.py [--rounds 5] [--reps 10] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import murcl_amd  # noqa: E402
from murcl_amd import ops  # noqa: E402


def window_ms(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def compare(name, fn, rounds, reps):
    res = {}
    for det in (False, True):                                   # warm every shape in both modes (workspaces, code objects)
        with murcl_amd.deterministic(det):
            for _ in range(3):
                fn()
            c0 = ops.float_atomic_launches()
            fn()
            res[det] = dict(order_dependent_launches_per_pass=ops.float_atomic_launches() - c0, windows=[])
    for _ in range(rounds):
        for det in (False, True):
            with murcl_amd.deterministic(det):
                res[det]["windows"].append(window_ms(fn, reps))
    out = {}
    for det, key in ((False, "default"), (True, "deterministic")):
        w = sorted(res[det]["windows"])
        out[key] = dict(ms=round(w[len(w) // 2], 4), min=round(w[0], 4), max=round(w[-1], 4),
                        order_dependent_launches_per_pass=res[det]["order_dependent_launches_per_pass"])
    out["ratio"] = round(out["deterministic"]["ms"] / out["default"]["ms"], 4)
    print(json.dumps({name: out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured on a CPU"
    dev = torch.device("cuda:0")
    out = {}

    model, fc, opt, crit = bench.build(torch.bfloat16, dev, 64)
    views = bench.synth_views(64, 2048, 512, torch.bfloat16, dev, 0)
    out["c2_bf16_step_64x2048x512"] = compare("c2_bf16_step_64x2048x512", bench.make_step(model, fc, opt, crit, views, 1), a.rounds, a.reps)
    del model, fc, opt, crit, views

    from murcl_amd.models.clam import CLAM_SB
    from murcl_amd.models.dsmil import build_dsmil
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    m = CLAM_SB(gate=True, size_arg="small", dropout=True, k_sample=8, n_classes=2, subtyping=True, in_dim=512).to(dev).eval()
    m.compute_dtype = torch.bfloat16
    for p in m.parameters():
        ops.manage_param(p)
    x = (torch.randn((64, 4096, 512), generator=g, device=dev).abs() * 0.5).bfloat16()
    labels = torch.randint(0, 2, (64,), generator=torch.Generator().manual_seed(1)).to(dev)

    def clam_fb():
        for p in m.parameters():
            p.grad = None
        M, _, _, il, _, _ = m._run(x, labels, True)
        torch.autograd.backward((M, il), [bench._ones_like(M), bench._ones_like(il)])
    out["clam_sb_c3_fwd_bwd_instance_loss"] = compare("clam_sb_c3_fwd_bwd_instance_loss", clam_fb, a.rounds, a.reps)
    del m, x

    md = build_dsmil(1024, 2).to(dev)
    for p in md.parameters():
        ops.manage_param(p)
    xd = torch.randn((16, 8192, 1024), generator=g, device=dev).abs() * 0.5

    def dsmil_fb():
        for p in md.parameters():
            p.grad = None
        classes, bag, cmax = md._run(xd, want_max=True)
        torch.autograd.backward((bag, cmax), (bench._ones_like(bag), bench._ones_like(cmax)))
    out["dsmil_c5_share_fwd_bwd"] = compare("dsmil_c5_share_fwd_bwd", dsmil_fb, a.rounds, a.reps)
    del md, xd

    A, B = torch.randn((33, 1536), device=dev), torch.randn((40, 1536), device=dev)
    out["gemm_nt_33x40x1536_f32"] = compare("gemm_nt_33x40x1536_f32", lambda: ops.gemm_nt(A, B), a.rounds, 200)
    # bag-level weight gradients off the headline shape: ATOMIC by default, PARTS (partial tiles + a reduce launch) in the mode
    for name, dt_, (M, N1, N2) in (("gemm_tn_768x3072x512_f32", torch.float32, (768, 3072, 512)),
                                   ("gemm_tn_4096x128x512_bf16", torch.bfloat16, (4096, 128, 512)),
                                   ("gemm_tn_4096x256x128_bf16_wide", torch.bfloat16, (4096, 256, 128))):
        At, Bt = torch.randn((M, N1), device=dev).to(dt_), torch.randn((M, N2), device=dev).to(dt_)
        Ct = torch.zeros((N1, N2), device=dev)
        out[name] = compare(name, lambda: ops.gemm_tn(At, Bt, out=Ct), a.rounds, 100)
    # one native PPO epoch over the entry script's default rollout: T = 6 x 128 bags = 768 rows, S = H = 512, K = 10
    from murcl_amd.models.rlmil import ActorCritic
    pol = ActorCritic(512, 512, 512, False, action_std=0.5, action_size=10).to(dev)
    for p in pol.parameters():
        p.grad = torch.zeros_like(p)
    st, ac = torch.randn((6, 128, 512), device=dev), torch.rand((6, 128, 10), device=dev)
    olp, ret = torch.randn((6, 128), device=dev) * 0.1 - 5.0, torch.randn((6, 128), device=dev)
    ptab, gtab = pol.pointer_table(), pol.pointer_table(grads=True)
    out["ppo_epoch_768_rows"] = compare("ppo_epoch_768_rows", lambda: ops.ppo_epoch(ptab, gtab, 512, 512, 10, st, ac, olp, ret, 768, 0.5, 0.2, 0.0),
                                        a.rounds, 20)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
