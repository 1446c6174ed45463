#!/usr/bin/env python3
"""IndexFlat::range_search on the flat 1M shape.

10 000 queries x 1M float_rand rows x d = 128, L2, one GPU: the library's
"flat_range" timer (both passes, HIP events) and the host wall time of the
call, at a radius with about 10 hits per query (the 2000th smallest of the 64
nearest distances of 200 sample queries) and at one with none; for scale
IndexFlat.search(k = 1) on the same data.

    python scripts/exp_flat_range.py [--nb 1000000] [--nq 10000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def timed(idx, name, fn, reps):
    out = []
    for _ in range(reps):
        idx.reset_kernel_times()
        t0 = time.perf_counter()
        res = fn()
        wall = (time.perf_counter() - t0) * 1e3
        kt = idx.kernel_times()
        out.append({"wall_ms": wall,
                    "kernel_ms": sum(t[1] for t in kt if t[0] == name),
                    "stages": sorted({t[0] for t in kt})})
    return res, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1000000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    amd = ge.load_package()
    xb = amd.float_rand(a.nb * a.d, 1234).reshape(a.nb, a.d)
    xq = amd.float_rand(a.nq * a.d, 5678).reshape(a.nq, a.d)
    idx = amd.index_factory(a.d, "Flat")
    idx.add(xb)
    amd.set_kernel_timing(True)
    # the radius below which 200 sample queries have 10 neighbours each on
    # average (the median 10th-NN distance gives 23: the counts are skewed)
    Dk, _ = idx.search(xq[:200], 64)
    r_hits = float(np.sort(Dk.ravel())[200 * 10])
    r_none = float(Dk[:, 0].min()) * 0.5
    res = {"nb": a.nb, "nq": a.nq, "d": a.d, "flop_per_pass": 2.0 * a.nb * a.nq * a.d}
    idx.range_search(xq[:256], r_hits)  # warm-up (allocations, code load)
    for tag, r in (("hits", r_hits), ("none", r_none)):
        (lims, _, _), t = timed(idx, "flat_range", lambda: idx.range_search(xq, r), a.reps)
        res[tag] = {"radius": r, "hits_per_query": float(lims[-1]) / a.nq, "runs": t}
    _, t = timed(idx, "", lambda: idx.search(xq, 1), a.reps)
    for run in t:
        run.pop("kernel_ms")
    res["search_k1"] = {"runs": t}
    idx.reset_kernel_times()
    idx.search(xq, 1)
    res["search_k1"]["kernel_stages_ms"] = [[t[0], t[1]] for t in idx.kernel_times()]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
