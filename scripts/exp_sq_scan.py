#!/usr/bin/env python3
"""The IVF-SQ8 exact scan beside the IVF-Flat exact scan on the c2 shape:
IVF4096, d = 128, 1M float_rand vectors, 10k device-resident queries,
nprobe 32, k 10.  Both indexes share the coarse centroids (so the same lists
are probed) and run Index::search_device; IVF-Flat runs with
FAISS_AMD_IVF_SCAN=exact (scan_mode 1: kernels_exact.hip k_ex_flat), IVF-SQ8
runs kernels_sq.hip k_ex_sq.  Steps are timed with HIP events after a warm-up,
as bench.py does; the scan stage alone comes from the library's stage timers
("ivf_exact_scan": offsets + candidate pass + select).

Writes profiles/sq8_scan.json (or --out) and prints it.

    python scripts/exp_sq_scan.py [--steps 20] [--warmup 5]
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

PEAK_HBM_GBS = 8000.0  # as bench.py
PEAK_FP32_TFLOPS = 157.3


def stage_ms(index, steps):
    out = {}
    for nm, ms, _ in index.kernel_times():
        out[nm] = out.get(nm, 0.0) + ms / steps
    return out


def measure(amd, index, x_t, k, steps, warmup):
    n = x_t.shape[0]
    dev = x_t.device
    D_t = torch.empty((n, k), dtype=torch.float32, device=dev)
    I_t = torch.empty((n, k), dtype=torch.int64, device=dev)
    # a stream of its own: the library runs on the stream it is given (its
    # own when given the null stream), and the events must be on the same one
    ts = torch.cuda.Stream(device=dev)
    stream = ts.cuda_stream
    assert stream != 0

    def step():
        index.search_device(n, x_t.data_ptr(), k, D_t.data_ptr(), I_t.data_ptr(), stream)
    torch.cuda.synchronize()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ts)
    for _ in range(steps):
        step()
    e1.record(ts)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    # the stages, in a second pass with every stage timed
    amd.set_kernel_timing(True)
    index.reset_kernel_times()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    amd.set_kernel_timing(False)
    return ms, stage_ms(index, steps), D_t.cpu().numpy(), I_t.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq8_scan.json"))
    args = ap.parse_args()
    assert args.steps >= 20 or args.nb < 1_000_000, "at least 20 timed steps"
    d, nlist, nprobe, k, ntrain = 128, 4096, 32, 10, 200_000
    nb, nq = args.nb, args.nq
    amd = ge.load_package()
    torch.cuda.set_device(0)
    amd.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    xb = amd.float_rand(nb * d, 1234).reshape(nb, d)
    xq = amd.float_rand(nq * d, 5678).reshape(nq, d)
    flat = amd.index_factory(d, f"IVF{nlist},Flat")
    flat.train(xb[:ntrain])
    flat.add(xb)
    flat.nprobe = nprobe
    sq = amd.index_factory(d, f"IVF{nlist},SQ8")
    sq.quantizer.add(flat.quantizer.xb)  # the same lists; train() skips k-means
    sq.train(xb[:100_000])               # (the reference's train_encoder_num_vectors)
    sq.add(xb)
    sq.nprobe = nprobe
    for ix in (flat, sq):
        ix.sync_device()
    print(f"built in {time.time() - t0:.1f}s", flush=True)
    sizes_equal = all(flat.get_list_size(l) == sq.get_list_size(l) for l in range(nlist))
    # rows scanned per step, counted as the reference counts them (ndis)
    st = amd.cvar.indexIVF_stats
    st.reset()
    sq.search(xq, k)
    rows = int(st.ndis)
    x_t = torch.from_numpy(xq).to(dev)
    os.environ["FAISS_AMD_IVF_SCAN"] = "exact"
    f_ms, f_st, _, If = measure(amd, flat, x_t, k, args.steps, args.warmup)
    del os.environ["FAISS_AMD_IVF_SCAN"]
    s_ms, s_st, _, Is = measure(amd, sq, x_t, k, args.steps, args.warmup)
    agree = float(np.mean([len(np.intersect1d(a, b)) for a, b in zip(If[:1000], Is[:1000])])) / k

    def leg(name, kernel, ms, stages, row_bytes, flop_per_comp):
        scan = stages.get("ivf_exact_scan", float("nan"))
        by = rows * row_bytes
        return {"index": name, "kernel": kernel, "ms_per_step": ms,
                "queries_per_s": nq / (ms * 1e-3), "stage_ms_per_step": stages,
                "ivf_exact_scan_ms": scan, "code_bytes_per_row": row_bytes,
                "code_bytes_per_step": by,
                "code_gbs_over_scan_stage": by / (scan * 1e-3) / 1e9,
                "frac_hbm_peak": by / (scan * 1e-3) / 1e9 / PEAK_HBM_GBS,
                "vector_ops_per_component": flop_per_comp,
                "vector_tops_over_scan_stage": rows * d * flop_per_comp / (scan * 1e-3) / 1e12,
                "frac_fp32_vector_peak": rows * d * flop_per_comp / (scan * 1e-3) / 1e12 /
                (PEAK_FP32_TFLOPS / 2)}

    out = {
        "shape": {"nlist": nlist, "d": d, "nb": nb, "nq": nq, "nprobe": nprobe, "k": k,
                  "steps": args.steps, "warmup": args.warmup, "same_lists": sizes_equal},
        "rows_scanned_per_step": rows,
        # Flat: subtract + fma per component; SQ8: convert, 2 fma (decode,
        # reconstruct), subtract, fma.  Peak for comparison: one vector
        # instruction per lane and clock = half the fp32 fma FLOP peak.
        "flat_exact": leg(f"IVF{nlist},Flat scan_mode=1", "k_ex_flat<true>", f_ms, f_st, 4 * d, 2),
        "sq8": leg(f"IVF{nlist},SQ8", "k_ex_sq<true, QT_8bit>", s_ms, s_st, d, 5),
        "top10_overlap_flat_vs_sq8": agree,
        "device": torch.cuda.get_device_name(0),
    }
    txt = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
