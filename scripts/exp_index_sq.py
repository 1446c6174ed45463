#!/usr/bin/env python3
"""Times IndexScalarQuantizer's full scan (kern::sq_flat_search) on the GPU.

SQ8 and SQfp16 (L2) over 1M random codes, d = 128, k = 10, with 64 and 10k
device-resident queries, and IndexFlat (L2) on the same shape in the same run
as the yardstick: Index::search_device in HIP-event windows of `steps` calls
after a warm-up, on a stream of the script's own, the three indexes taking
turns in every repeat; min / median / max are kept.  A second pass with the
library's per-stage HIP events on gives the split of an SQ search into the
scan kernel and the exact select (summed over the query chunks of one call).
Beside the measured times stand the figures the shape gives (modelled, not
measured): code bytes read per row, 2 d vector operations per (query, row)
pair for L2, 4 bytes of dense distance written per pair.  Ranges and codes are
random (no training): the kernel's time does not depend on their values.
Writes profiles/index_sq.json (or --out).

    python scripts/exp_index_sq.py [--steps 10] [--warmup 3] [--nb 1000000]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_sq.json"))
    args = ap.parse_args()
    amd = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("exp_index_sq.py needs a GPU")
    ts = torch.cuda.Stream()
    d, k, nb = 128, 10, args.nb
    rng = np.random.default_rng(1)
    sq8 = amd.IndexScalarQuantizer(d, amd.QT_8bit)
    sq8.set_content(np.concatenate([rng.standard_normal(d), rng.uniform(0.5, 3, d)]),
                    rng.integers(0, 256, (nb, d), dtype=np.uint8))
    fp16 = amd.IndexScalarQuantizer(d, amd.QT_fp16)
    fp16.set_content(None, np.ascontiguousarray(
        rng.standard_normal((nb, d), dtype=np.float32).astype("<f2")).view(np.uint8))
    flat = amd.IndexFlat(d)
    flat.add(rng.standard_normal((nb, d), dtype=np.float32))
    indexes = (("SQ8", sq8, d), ("SQfp16", fp16, 2 * d), ("Flat", flat, 4 * d))
    rows = []
    for nq in (64, 10000):
        x = torch.from_numpy(rng.standard_normal((nq, d)).astype(np.float32)).cuda()
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        steps = max(1, args.steps // 5) if nq >= 10000 else args.steps
        # kern::sq_flat_query_chunk: 256 MiB of dense rows, whole 64-query tiles
        chunk = (1 << 26) // nb
        chunk = max(1, min(nq, chunk // 64 * 64 if chunk >= 64 else chunk))

        def call(idx):
            idx.search_device(nq, x.data_ptr(), k, D.data_ptr(), I.data_ptr(), stream=ts.cuda_stream)
        for _, idx, _ in indexes:
            for _ in range(args.warmup):
                call(idx)
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in indexes}
        for _ in range(args.repeats):
            for name, idx, _ in indexes:
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record(ts)
                for _ in range(steps):
                    call(idx)
                e1.record(ts)
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / steps)
        amd.set_kernel_timing(True)
        split = {}
        for name, idx, _ in indexes[:2]:
            idx.reset_kernel_times()
            call(idx)
            torch.cuda.synchronize()
            split[name] = {}
            for stage, t, _ in idx.kernel_times():
                split[name][stage] = split[name].get(stage, 0.0) + t
        amd.set_kernel_timing(False)
        for name, _, row_bytes in indexes:
            rows.append(dict(index=name, nb=nb, nq=nq, k=k, d=d, measured=dict(
                ms_min=min(ms[name]), ms_median=float(np.median(ms[name])), ms_max=max(ms[name]),
                stage_ms=split.get(name)), modelled=dict(
                code_bytes_per_row=row_bytes, vector_ops_per_pair=2 * d,
                dense_bytes_written_per_pair=4 if name != "Flat" else None,
                query_chunks=-(-nq // chunk) if name != "Flat" else None)))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), steps=args.steps,
                       warmup=args.warmup, repeats=args.repeats, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
