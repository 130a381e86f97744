"""GPU time of one Lloyd iteration on the two k-means entries, beside a plain copy of the same X.

    python tools/kmeans_wide_time.py [--rows 20000] [--reps 200] [--windows 7] [--warmup 30] [--out FILE]

Device events around ``reps`` back-to-back calls; the median of ``windows`` such windows after ``warmup`` calls.  Per shape one JSON
line: the copy of X (murcl_calib_copy: read + write, 16-byte accesses), each entry's time, and the copy's time over the entry's time
("fraction_of_copy").  Shapes: (d, K) = (1024, 10) on both entries - the narrow kernel is the baseline -, (2048, 10) and (512, 40)
on the wide entry alone.  A last line times a 1 GiB copy: the rate past the Infinity Cache, for scale."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from murcl_amd import _lib  # noqa: E402
from murcl_amd._lib import check, ptr, stream  # noqa: E402


def median_us(fn, reps, windows, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / reps)
    times.sort()
    return {"median_us": round(times[len(times) // 2], 2), "min_us": round(times[0], 2), "max_us": round(times[-1], 2)}


def shape(L, dev, N, d, K, entries, args):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    blobs = torch.randn((K, d), generator=g, device=dev) * 2
    X = (blobs[torch.randint(K, (N,), generator=g, device=dev)] + 0.5 * torch.randn((N, d), generator=g, device=dev)).contiguous()
    Y = torch.empty_like(X)
    nbytes = X.numel() * 4
    copy = median_us(lambda: check(L.murcl_calib_copy(ptr(X), ptr(Y), nbytes, stream()), "calib_copy"), args.reps, args.windows, args.warmup)
    out = {"N": N, "d": d, "K": K, "X_MB": round(nbytes / 1e6, 2), "copy": copy, "copy_TBps": round(2 * nbytes / copy["median_us"] / 1e6, 2)}
    for name in entries:
        fn = getattr(L, name)
        query = L.murcl_kmeans_workspace_bytes if name == "murcl_kmeans_step" else L.murcl_kmeans_wide_workspace_bytes
        centers = blobs.clone()
        labels = torch.full((N,), -1, dtype=torch.int32, device=dev)
        counts = torch.empty((K,), dtype=torch.int32, device=dev)
        mind2 = torch.empty((N,), device=dev)
        stats = torch.zeros((3 + K,), device=dev)
        ws = torch.empty((query(N, d, K) + 3) // 4, device=dev)

        def step():
            check(fn(ptr(X), N, d, K, ptr(centers), ptr(labels), ptr(counts), ptr(stats), ptr(mind2), 1, ptr(ws), stream()), name)
        r = median_us(step, args.reps, args.windows, args.warmup)
        r["fraction_of_copy"] = round(copy["median_us"] / r["median_us"], 3)
        out[name] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the lines to this file as one JSON list")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_wide_time: needs the GPU (a CPU timing says nothing about it)")
    L, dev = _lib.lib(), torch.device("cuda:0")
    res = []
    for d, K, entries in [(1024, 10, ["murcl_kmeans_step", "murcl_kmeans_step_wide"]), (2048, 10, ["murcl_kmeans_step_wide"]),
                          (512, 40, ["murcl_kmeans_step_wide"])]:
        res.append(shape(L, dev, args.rows, d, K, entries, args))
        print(json.dumps(res[-1]), flush=True)
    big = torch.empty((1 << 28,), device=dev).normal_()
    bigY = torch.empty_like(big)
    c = median_us(lambda: check(L.murcl_calib_copy(ptr(big), ptr(bigY), 1 << 30, stream()), "calib_copy"), 20, 5, 3)
    res.append({"copy_1GiB": c, "copy_TBps": round(2 * (1 << 30) / c["median_us"] / 1e6, 2)})
    print(json.dumps(res[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
