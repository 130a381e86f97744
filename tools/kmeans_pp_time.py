"""GPU time of one k-means++ seeding: the scikit-learn-stream seeding on its own launches (murcl_kmeans_pp) beside the native
torch-op ``kmeans_plusplus``.

    python tools/kmeans_pp_time.py [--rows 20000] [--reps 20] [--windows 7] [--warmup 5] [--out FILE]

Same process, the two seedings interleaved window by window, device events around ``reps`` back-to-back seedings, the median of
``windows`` such windows after ``warmup`` seedings each.  The native seeding ends every one of its K-1 steps in a host sync, so its
window is wall time on the device clock; the new one is enqueued whole (its draws are taken on the host before the window starts, and
its indices are not read back inside it).  Shapes: N rows x d in (512, 2048), K = 10.  One JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from murcl_amd.utils import clustering as C  # noqa: E402


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def summary(times):
    times = sorted(times)
    return {"median_us": round(times[len(times) // 2], 1), "min_us": round(times[0], 1), "max_us": round(times[-1], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file as one JSON list")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_pp_time: needs the GPU (a CPU timing says nothing about it)")
    dev, K, res = torch.device("cuda:0"), 10, []
    for d in (512, 2048):
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        blobs = torch.randn((K, d), generator=g, device=dev) * 2
        X = (blobs[torch.randint(K, (args.rows,), generator=g, device=dev)] + torch.randn((args.rows, d), generator=g, device=dev)).contiguous()
        first, uniforms = C.sklearn_draws(np.random.RandomState(985), args.rows, K)
        u = torch.from_numpy(uniforms.reshape(-1)).to(dev)
        L = C._lib.lib()
        indices = torch.empty((K,), dtype=torch.int32, device=dev)
        centers = torch.empty((K, d), device=dev)
        ws = torch.empty(((L.murcl_kmeans_pp_workspace_bytes(args.rows, d, K) + 15) // 16, 2), dtype=torch.float64, device=dev)

        def new():
            C.check(L.murcl_kmeans_pp(C.ptr(X), args.rows, d, K, first, C.ptr(u), C.ptr(indices), C.ptr(centers), C.ptr(ws), C.stream()), "kmeans_pp")

        def native():
            C.kmeans_plusplus(X, K, g)

        for fn in (new, native):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t = {"new": [], "native": []}
        for _ in range(args.windows):                                # interleaved: drift of the clocks lands on both
            t["new"].append(window_us(new, args.reps))
            t["native"].append(window_us(native, args.reps))
        line = {"N": args.rows, "d": d, "K": K, "murcl_kmeans_pp": summary(t["new"]), "kmeans_plusplus_native": summary(t["native"])}
        line["native_over_new"] = round(line["kmeans_plusplus_native"]["median_us"] / line["murcl_kmeans_pp"]["median_us"], 2)
        res.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
