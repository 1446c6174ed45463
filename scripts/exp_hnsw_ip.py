#!/usr/bin/env python3
"""Time of an inner-product IndexHNSWFlat on the c4 quantizer shape (HNSW32
over 16384 float_rand vectors of d = 128, 10k device-resident queries; the
shape of scripts/exp_hnsw_params.py) beside an L2 index over the same rows,
at efSearch 16 / 64 / 128 (k = min(efSearch, 64)).

Timed in one process with HIP events after a warm-up, in alternating rounds
(every variant once per round; the median over the rounds with the min and max):
  ip            the inner-product index, default mode: the register kernel
                without int8 image and replay log (ef <= 64), the sequential
                kernel (ef 128)
  l2_default    the L2 index, default mode: the fast kernels (register kernel
                with int8 image and replay log; the batched kernel at ef 128)
  l2_same_form  the L2 index through the form `ip` runs: FAISS_AMD_HNSW_Q8=0
                (read when the index is uploaded) and FAISS_AMD_HNSW_REPLAY=0
                for ef <= 64, FAISS_AMD_HNSW_EXACT=1 at ef 128
  l2_sel_all    the L2 index under a selector admitting every id: the
                sequential kernel's EXT form at every ef
The rows are centred (float_rand - 0.5) so that inner products have both
signs; the graphs differ with the metric, so the figures compare the work of
a search on each index, not one traversal under two formulas.

Writes profiles/hnsw_ip_c4q.json (or --out) and prints it.

    python scripts/exp_hnsw_ip.py [--rounds 7] [--index-l2 FILE --index-ip FILE]
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--index-l2", default=None,
                    help="index files of this shape written by an earlier run (the serial host "
                         "build of a graph takes minutes); built and written when missing")
    ap.add_argument("--index-ip", default=None)
    ap.add_argument("--build-only", action="store_true", help="write the index files and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_ip_c4q.json"))
    args = ap.parse_args()
    amd, orc = ge.load_package(), ge.load_oracle()
    d = 128
    xb = orc.float_rand(args.n * d, 1234).reshape(args.n, d) - np.float32(0.5)
    xq = orc.float_rand(args.nq * d, 5678).reshape(args.nq, d) - np.float32(0.5)

    def load(fn, metric):
        if fn and os.path.exists(fn):
            idx = amd.read_index(fn)
            assert idx.ntotal == args.n and idx.d == d and idx.metric_type == metric
            return idx
        idx = amd.IndexHNSWFlat(d, 32, metric)
        idx.add(xb)
        if fn:
            amd.write_index(idx, fn)
        return idx

    ip = load(args.index_ip, amd.METRIC_INNER_PRODUCT)
    l2 = load(args.index_l2, amd.METRIC_L2)
    if args.build_only:
        return
    ip.sync_device()
    l2.sync_device()
    os.environ["FAISS_AMD_HNSW_Q8"] = "0"  # (read at upload: this copy has no int8 image)
    l2_plain = load(args.index_l2, amd.METRIC_L2)
    l2_plain.sync_device()
    del os.environ["FAISS_AMD_HNSW_Q8"]
    ts = torch.cuda.Stream()
    x_t = torch.from_numpy(xq).cuda()
    sel = amd.IDSelectorRange(0, args.n)
    P = amd.SearchParametersHNSW
    variants = {}
    for ef in (16, 64, 128):
        k = min(ef, 64)
        same = {"FAISS_AMD_HNSW_REPLAY": "0"} if ef <= 64 else {"FAISS_AMD_HNSW_EXACT": "1"}
        variants[f"ip_ef{ef}"] = (ip, k, P(ef), {})
        variants[f"l2_default_ef{ef}"] = (l2, k, P(ef), {})
        variants[f"l2_same_form_ef{ef}"] = (l2_plain, k, P(ef), same)
        variants[f"l2_sel_all_ef{ef}"] = (l2, k, P(ef, sel=sel), {})
    D_t = torch.empty((args.nq, 64), dtype=torch.float32, device="cuda")
    I_t = torch.empty((args.nq, 64), dtype=torch.int64, device="cuda")

    def run(name, steps):
        idx, k, params, env = variants[name]
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

    counts = {}
    for name in variants:
        run(name, 2)  # warm-up of every variant
        # the work of a search, per query: distance computations and hops
        # (HNSWStats.ndis / nhops), and the share of queries the register
        # kernel searched a second time with the heap-layout form
        variants[name][0].fold_device_stats()
        amd.cvar.hnsw_stats.reset()
        run(name, 1)
        variants[name][0].fold_device_stats()
        hs = amd.cvar.hnsw_stats
        counts[name] = {"ndis": hs.ndis / args.nq, "nhops": hs.nhops / args.nq,
                        "searched_again": amd.cvar.hnsw_replay_stats[1] / args.nq}
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name in variants:
            times[name].append(run(name, args.steps))
    out = {"shape": {"ntotal": args.n, "d": d, "M": 32, "nq": args.nq,
                     "k": "min(efSearch, 64)"},
           "rounds": args.rounds, "steps_per_round": args.steps,
           "ms_per_batch": {n: {"median": float(np.median(t)), "min": float(min(t)),
                                "max": float(max(t))} for n, t in times.items()},
           "per_query": counts}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
