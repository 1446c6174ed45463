#!/usr/bin/env python3
"""Times IndexPQ's full scan (kern::pq_flat_search) on the GPU.

PQ32x8 and PQ32x4 over 1M random codes, d = 128, k = 10, with 1, 64 and 10k
device-resident queries: Index::search_device in HIP-event windows of `steps`
calls after a warm-up, on a stream of the script's own; every window is
repeated and min / median / max are kept.  Beside each time the two figures
the shape gives: the LDS lookups (rows x queries x M / QI reads of one table
entry per query of the group) and the code bytes read (codes x query groups).
Codebooks and codes are random (no training): the kernel's time does not
depend on their values.  Writes profiles/index_pq.json (or --out).

    python scripts/exp_index_pq.py [--steps 10] [--warmup 3] [--nb 1000000]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nb", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_pq.json"))
    args = ap.parse_args()
    amd = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("exp_index_pq.py needs a GPU")
    ts = torch.cuda.Stream()
    d, k, rows = 128, 10, []
    rng = np.random.default_rng(1)
    for M, nbits, QI in ((32, 8, 4), (32, 4, 8)):
        idx = amd.IndexPQ(d, M, nbits)
        cs = idx.code_size
        idx.set_content(rng.standard_normal((M, 1 << nbits, d // M)).astype(np.float32),
                        rng.integers(0, 256, (args.nb, cs), dtype=np.uint8))
        for nq in (1, 64, 10000):
            x = torch.from_numpy(rng.standard_normal((nq, d)).astype(np.float32)).cuda()
            D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            steps = max(1, args.steps // 5) if nq >= 10000 else args.steps

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
            qi = min(QI, 1 << max(0, (nq - 1).bit_length()))
            groups = -(-nq // qi)
            rows.append(dict(index=f"PQ{M}x{nbits}", nb=args.nb, nq=nq, k=k, QI=qi,
                             ms_min=min(ms), ms_median=float(np.median(ms)), ms_max=max(ms),
                             lds_lookups=args.nb * groups * M, code_bytes=args.nb * cs * groups))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), steps=args.steps,
                       warmup=args.warmup, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
