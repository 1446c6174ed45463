#!/usr/bin/env python3
"""Time of IndexHNSW's non-default search modes on the c4 quantizer shape:
HNSW32 over 16384 float_rand vectors of d = 128, 10k device-resident queries,
efSearch 64, k 64 (what IVF16384_HNSW32 asks of its quantizer at nprobe 64).

Timed in one process with HIP events after a warm-up, in alternating rounds
(every variant once per round, the median over the rounds reported with the
min and max):
  default      the default mode (register kernel), for scale
  default_seq  the default mode in the sequential kernel: FAISS_AMD_HNSW_WIDE=0
               and efSearch 129 > 128 keep the fast kernels away
  mode_a       check_relative_distance = false
  mode_b       bounded_queue = false
  sel10        the default mode under a selector of every tenth id
  mode_a_129   check_relative_distance = false at efSearch 129 (beside default_seq)
Also Mode B's queue scratch: the bytes reserved per query, and the high-water
mark of the unbounded queue over the first --model-queries queries from
tests/hnsw_params_model.py (8 bytes per entry; a CPU count, not a GPU reading).

Writes profiles/hnsw_params_c4q.json (or --out) and prints it.

    python scripts/exp_hnsw_params.py [--rounds 7] [--index FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--model-queries", type=int, default=100)
    ap.add_argument("--index", default=None,
                    help="an index file of this shape written by an earlier run (the serial "
                         "host build of the graph takes minutes); built and written when missing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_params_c4q.json"))
    args = ap.parse_args()
    amd, orc = ge.load_package(), ge.load_oracle()
    d, k, ef = 128, 64, 64
    xb = orc.float_rand(args.n * d, 1234).reshape(args.n, d)
    xq = orc.float_rand(args.nq * d, 5678).reshape(args.nq, d)
    if args.index and os.path.exists(args.index):
        idx = amd.read_index(args.index)
        assert idx.ntotal == args.n and idx.d == d
    else:
        idx = amd.IndexHNSWFlat(d, 32)
        idx.add(xb)
        if args.index:
            amd.write_index(idx, args.index)
    idx.sync_device()
    ts = torch.cuda.Stream()
    x_t = torch.from_numpy(xq).cuda()
    D_t = torch.empty((args.nq, k), dtype=torch.float32, device="cuda")
    I_t = torch.empty((args.nq, k), dtype=torch.int64, device="cuda")
    sel = amd.IDSelectorBatch(np.arange(0, args.n, 10, dtype=np.int64))
    P = amd.SearchParametersHNSW
    variants = {
        "default": (P(ef), {}),
        "default_seq": (P(129), {"FAISS_AMD_HNSW_WIDE": "0"}),
        "mode_a": (P(ef, check_relative_distance=False), {}),
        "mode_b": (P(ef, bounded_queue=False), {}),
        "sel10": (P(ef, sel=sel), {}),
        "mode_a_129": (P(129, check_relative_distance=False), {}),
    }

    def run(name, steps):
        params, env = variants[name]
        old = {e: os.environ.get(e) for e in env}
        os.environ.update(env)
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            for _ in range(steps):
                idx.search_device(args.nq, x_t.data_ptr(), k, D_t.data_ptr(), I_t.data_ptr(),
                                  ts.cuda_stream, params=params)
            e1.record(ts)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps
        finally:
            for e, v in old.items():
                if v is None:
                    os.environ.pop(e, None)
                else:
                    os.environ[e] = v

    for name in variants:
        run(name, 2)  # warm-up of every variant
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name in variants:
            times[name].append(run(name, args.steps))
    out = {"shape": {"ntotal": args.n, "d": d, "M": 32, "nq": args.nq, "efSearch": ef, "k": k},
           "rounds": args.rounds, "steps_per_round": args.steps,
           "ms_per_batch": {n: {"median": float(np.median(t)), "min": float(min(t)),
                                "max": float(max(t))} for n, t in times.items()}}
    import hnsw_params_model as hm
    m = hm.Model(orc, orc.HNSWGraph.from_index(idx))
    m.search(xq[:args.model_queries], k, ef, bounded_queue=False)
    out["mode_b_scratch"] = {
        "reserved_bytes_per_query": 8 * (min(ef, args.n) + args.n + 4),
        "queue_high_water_entries": int(m.queue_high_water),
        "queue_high_water_bytes": 8 * int(m.queue_high_water),
        "model_queries": args.model_queries,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
