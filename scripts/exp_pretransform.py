#!/usr/bin/env python3
"""What an IndexPreTransform front end costs on the GPU.

1. kern::linear_transform alone on device rows: 10k x 128 -> 128 and
   10k x 128 -> 64 (the tile the batch size selects), and the small batches
   n = 1 and n = 16 on both tile shapes (variant 1 = 128-row tile, 2 = 32-row
   tile), which give the same bits; the two are timed in alternating windows.
2. The c3 shape (IVF4096,PQ32, d = 128, 1M float_rand vectors, nprobe 32,
   k 10, 10k device-resident queries): Index::search_device of the IVF-PQ index
   on already transformed queries against the same index behind a 128 -> 128
   orthonormal front end on the raw queries, in alternating windows.

Times are HIP events around `steps` calls after a warm-up, on a stream of the
script's own, as bench.py does; every window is repeated and min / median /
max are kept.  Writes profiles/pretransform.json (or --out) and prints it.

    python scripts/exp_pretransform.py [--steps 20] [--warmup 5] [--nb 1000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def window(ts, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ts)
    for _ in range(calls):
        fn()
    e1.record(ts)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls  # ms per call


def alternate(ts, legs, calls, warmup, reps):
    """legs: {name: fn}.  reps windows of each, interleaved; ms per call."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {nm: [] for nm in legs}
    for _ in range(reps):
        for nm, fn in legs.items():
            got[nm].append(window(ts, fn, calls))
    return {nm: {"min_ms": min(v), "median_ms": float(np.median(v)), "max_ms": max(v)}
            for nm, v in got.items()}


def kernel_legs(amd, ts, dev, n, d_in, d_out, variants):
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((n, d_in)).astype(np.float32)).to(dev)
    A = torch.from_numpy(rng.standard_normal((d_out, d_in)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rng.standard_normal(d_out).astype(np.float32)).to(dev)
    y = torch.empty((n, d_out), dtype=torch.float32, device=dev)
    keep = (x, A, b, y)

    def leg(v):
        return lambda: amd.linear_transform_device(x.data_ptr(), n, d_in, A.data_ptr(), d_in,
                                                   d_out, b.data_ptr(), y.data_ptr(), d_out,
                                                   variant=v, stream=ts.cuda_stream)
    return {f"variant{v}": leg(v) for v in variants}, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretransform.json"))
    args = ap.parse_args()
    amd = ge.load_package()
    assert amd.device_count() >= 1, "needs a HIP device"
    torch.cuda.set_device(0)
    amd.set_device(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "reps": args.reps,
           "kernel": {}}

    # 1. the kernel alone; 200 calls a window so that a window is not a few microseconds
    for n, d_in, d_out, variants in [(args.nq, 128, 128, (0,)), (args.nq, 128, 64, (0,)),
                                     (1, 128, 128, (1, 2)), (16, 128, 128, (1, 2)),
                                     (1, 128, 64, (1, 2)), (16, 128, 64, (1, 2))]:
        legs, keep = kernel_legs(amd, ts, dev, n, d_in, d_out, variants)
        res = alternate(ts, legs, 200, 20, args.reps)
        for r in res.values():
            r["gflops"] = 2.0 * n * d_in * d_out / (r["median_ms"] * 1e-3) / 1e9
            r["gbs"] = 4.0 * (n * (d_in + d_out) + d_in * d_out) / (r["median_ms"] * 1e-3) / 1e9
        out["kernel"][f"{n}x{d_in}->{d_out}"] = res
        print(n, d_in, d_out, res, flush=True)

    # 2. the c3 shape with and without a front end
    d, nlist, nprobe, k, M = 128, 4096, 32, 10, 32
    nb, nq = args.nb, args.nq
    ntrain = min(nb, 200_000)
    t0 = time.time()
    xb = amd.float_rand(nb * d, 1234).reshape(nb, d)
    xq = amd.float_rand(nq * d, 5678).reshape(nq, d)
    q, _ = np.linalg.qr(np.random.default_rng(2).standard_normal((d, d)))
    lt = amd.LinearTransform(A=q.astype(np.float32))
    base = amd.index_factory(d, f"IVF{nlist},PQ{M}")
    idx = amd.IndexPreTransform(lt, base)
    idx.train(xb[:ntrain])
    idx.add(xb)
    base.nprobe = nprobe
    idx.sync_device()
    print(f"built in {time.time() - t0:.1f}s", flush=True)
    xt = idx.apply_chain(xq)
    x_t, xt_t = torch.from_numpy(xq).to(dev), torch.from_numpy(xt).to(dev)
    D1 = torch.empty((nq, k), dtype=torch.float32, device=dev)
    I1 = torch.empty((nq, k), dtype=torch.int64, device=dev)
    D2, I2 = torch.empty_like(D1), torch.empty_like(I1)
    legs = {
        "base_on_transformed": lambda: base.search_device(nq, xt_t.data_ptr(), k, D1.data_ptr(),
                                                          I1.data_ptr(), ts.cuda_stream),
        "pretransform": lambda: idx.search_device(nq, x_t.data_ptr(), k, D2.data_ptr(),
                                                  I2.data_ptr(), ts.cuda_stream),
    }
    res = alternate(ts, legs, args.steps, args.warmup, args.reps)
    same = bool(torch.equal(I1, I2) and torch.equal(D1.view(torch.int32), D2.view(torch.int32)))
    extra = res["pretransform"]["median_ms"] - res["base_on_transformed"]["median_ms"]
    out["c3"] = {"shape": {"nlist": nlist, "d": d, "M": M, "nb": nb, "nq": nq, "nprobe": nprobe,
                           "k": k},
                 "ms_per_search": res, "results_identical": same,
                 "front_end_ms": extra,
                 "front_end_share_of_search": extra / res["pretransform"]["median_ms"]}
    for nsmall in (1, 16):
        legs = {
            "base_on_transformed": lambda: base.search_device(
                nsmall, xt_t.data_ptr(), k, D1.data_ptr(), I1.data_ptr(), ts.cuda_stream),
            "pretransform": lambda: idx.search_device(
                nsmall, x_t.data_ptr(), k, D2.data_ptr(), I2.data_ptr(), ts.cuda_stream),
        }
        out["c3"][f"ms_per_search_n{nsmall}"] = alternate(ts, legs, 200, 20, args.reps)
    txt = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
