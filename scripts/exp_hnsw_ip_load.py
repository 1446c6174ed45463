#!/usr/bin/env python3
"""Where the register kernel's inner-product excess on the c4 quantizer shape
comes from (scripts/exp_hnsw_ip.py has the headline figures): the
inner-product index and the L2 index through the same kernel form
(FAISS_AMD_HNSW_Q8=0, FAISS_AMD_HNSW_REPLAY=0), efSearch = k = 16 and 64, at
2500 / 10000 / 40000 device-resident queries (the 10k set tiled), with the
host's enqueue time per call beside the HIP-event time.

--pmc-run: three calls per variant at 10k queries and nothing else, for a
counter run of its own, e.g.
    rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --kernel-include-regex k_hnsw_exact_reg \\
        --output-format csv -d out -o pmc -- python scripts/exp_hnsw_ip_load.py --pmc-run ...
(the kernel names carry the metric: the last template argument is IP).

Writes profiles/hnsw_ip_c4q_load.json (or --out) and prints it.

    python scripts/exp_hnsw_ip_load.py --index-l2 FILE --index-ip FILE
(the index files scripts/exp_hnsw_ip.py writes)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-l2", required=True)
    ap.add_argument("--index-ip", required=True)
    ap.add_argument("--pmc-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_ip_c4q_load.json"))
    args = ap.parse_args()
    amd, orc = ge.load_package(), ge.load_oracle()
    d = 128
    xq0 = orc.float_rand(10000 * d, 5678).reshape(10000, d) - np.float32(0.5)
    ip = amd.read_index(args.index_ip)
    ip.sync_device()
    os.environ["FAISS_AMD_HNSW_Q8"] = "0"  # (read at upload)
    l2 = amd.read_index(args.index_l2)
    l2.sync_device()
    os.environ["FAISS_AMD_HNSW_REPLAY"] = "0"
    ts = torch.cuda.Stream()
    out = {}
    for nq in ((10000,) if args.pmc_run else (2500, 10000, 40000)):
        x_t = torch.from_numpy(np.ascontiguousarray(np.tile(xq0, (4, 1))[:nq])).cuda()
        D_t = torch.empty((nq, 64), dtype=torch.float32, device="cuda")
        I_t = torch.empty((nq, 64), dtype=torch.int64, device="cuda")
        for ef in (16, 64):
            for name, idx in (("ip", ip), ("l2", l2)):
                p = amd.SearchParametersHNSW(ef)

                def call():
                    idx.search_device(nq, x_t.data_ptr(), ef, D_t.data_ptr(), I_t.data_ptr(),
                                      ts.cuda_stream, params=p)
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                if args.pmc_run:
                    continue
                ev, host = [], []
                for _ in range(5):
                    e0, e1 = (torch.cuda.Event(enable_timing=True),
                              torch.cuda.Event(enable_timing=True))
                    e0.record(ts)
                    t0 = time.perf_counter()
                    for _ in range(5):
                        call()
                    host.append((time.perf_counter() - t0) / 5 * 1e3)
                    e1.record(ts)
                    torch.cuda.synchronize()
                    ev.append(e0.elapsed_time(e1) / 5)
                out[f"{name}_ef{ef}_nq{nq}"] = {"event_ms": float(np.median(ev)),
                                               "host_enqueue_ms": float(np.median(host))}
    if args.pmc_run:
        return
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
