#!/usr/bin/env python3
"""Times the binary indexes' scans (kernels_binary.hip) on the GPU.

1M random rows of 256 bits, k = 10: IndexBinaryFlat and BIVF4096 (centroids =
4096 of the rows, nprobe 32) with 1, 64 and 10k device-resident queries,
IndexBinary.search_device in HIP-event windows of `steps` calls after a
warm-up, on a stream of the script's own; every window is repeated and min /
median / max are kept.  Beside each time the two bounds the shape gives: 2
VALU operations per dword and pair over 3.9e13 lane-ops/s, and the row bytes
read from memory (once per query tile for the flat scan, once per (query,
probe) for the IVF scan) over 8 TB/s.  The first query's flat result is checked
against numpy.  Writes profiles/binary.json (or --out).

    python scripts/exp_binary.py [--steps 500] [--warmup 3] [--nb 1000000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

VALU_OPS, HBM_BYTES = 256 * 4 * 16 * 2.4e9, 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nb", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binary.json"))
    args = ap.parse_args()
    amd = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("exp_binary.py needs a GPU")
    ts = torch.cuda.Stream()
    d, k, nlist, nprobe, rows = 256, 10, 4096, 32, []
    cs, W = d // 8, d // 32
    rng = np.random.default_rng(1)
    xb = rng.integers(0, 256, (args.nb, cs), dtype=np.uint8)
    xq_all = rng.integers(0, 256, (10000, cs), dtype=np.uint8)
    flat = amd.IndexBinaryFlat(d)
    flat.add(xb)
    quant = amd.IndexBinaryFlat(d)
    quant.add(xb[:nlist])
    ivf = amd.IndexBinaryIVF(quant, d, nlist)
    ivf.is_trained = True
    ivf.add(xb)
    ivf.nprobe = nprobe
    # one query against numpy: the k smallest by (distance, id)
    D1, I1 = flat.search(xq_all[:1], k)
    dis = np.unpackbits(xb ^ xq_all[:1], axis=1).sum(axis=1).astype(np.int32)
    order = np.lexsort((np.arange(args.nb), dis))[:k]
    assert np.array_equal(I1[0], order) and np.array_equal(D1[0], dis[order]), (D1, I1)
    print("flat result of query 0 equals numpy:", D1[0].tolist(), I1[0].tolist(), flush=True)
    for name, idx in (("BFlat", flat), (f"BIVF{nlist},nprobe{nprobe}", ivf)):
        for nq in (1, 64, 10000):
            x = torch.from_numpy(xq_all[:nq].copy()).cuda()
            D = torch.empty((nq, k), dtype=torch.int32, device="cuda")
            I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            # windows of a few tenths of a second at least: fewer calls where one is long
            steps = max(1, args.steps // (20 if idx is flat else 2)) if nq >= 10000 else args.steps

            def call():
                idx.search_device(nq, x.data_ptr(), k, D.data_ptr(), I.data_ptr(),
                                  stream=ts.cuda_stream)
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.repeats):
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record(ts)
                for _ in range(steps):
                    call()
                e1.record(ts)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / steps)
            if idx is flat:
                pairs, row_reads = args.nb * nq, args.nb * -(-nq // 16)
            else:  # coarse scan + the probed lists at their mean length
                pairs = nq * (nlist + nprobe * args.nb / nlist)
                row_reads = nlist * -(-nq // 16) + nq * nprobe * args.nb / nlist
            rows.append(dict(index=name, nb=args.nb, d=d, nq=nq, k=k, ms_min=min(ms),
                             ms_median=float(np.median(ms)), ms_max=max(ms),
                             valu_bound_ms=1e3 * pairs * 2 * W / VALU_OPS,
                             hbm_bound_ms=1e3 * row_reads * cs / HBM_BYTES))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), steps=args.steps,
                       warmup=args.warmup, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
