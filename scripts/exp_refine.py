#!/usr/bin/env python3
"""What IndexRefineFlat adds to an IVF-PQ search on the c3 shape: IVF4096,PQ32,
d = 128, 1M float_rand vectors, 10k device-resident queries, nprobe 32, k 10.

For k_factor in {1, 4, 16} the base index's search_device at k_base = k *
k_factor and the wrapper's search_device at k are timed in one process, in
alternating blocks, with HIP events after a warm-up (as bench.py times its
steps).  The wrapper adds only the refine stage (kernels_refine.hip + the exact
select) to the base search, so the base search at k_base on the same build is
its yardstick.  Reported per k_factor:
  * ms per step of both, and the library's "refine" stage timer;
  * the refine stage's byte MODEL nq * k_base * (4 d + 12) (the candidate rows,
    their labels and keys; not a counter reading) over that time, as a share of
    the HBM peak bench.py uses;
  * 10-recall@10 against an exact IndexFlat, for the base index and the wrapper;
  * the reference's IndexRefineFlat::search of the same index file on 16 CPU
    threads (oracle/reflib.py), when oracle/_ref is present.

Writes profiles/refine_c3.json (or --out) and prints it.

    python scripts/exp_refine.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

PEAK_HBM_GBS = 8000.0  # as bench.py


def timed(index, x_t, k, D_t, I_t, ts, steps):
    n = x_t.shape[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ts)
    for _ in range(steps):
        index.search_device(n, x_t.data_ptr(), k, D_t.data_ptr(), I_t.data_ptr(), ts.cuda_stream)
    e1.record(ts)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def recall_at_10(I, Igt):
    return float(np.mean([len(np.intersect1d(a, b)) for a, b in zip(I, Igt)])) / Igt.shape[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--ref-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_c3.json"))
    args = ap.parse_args()
    d, nlist, nprobe, k, ntrain = 128, 4096, 32, 10, 200_000
    nb, nq = args.nb, args.nq
    amd = ge.load_package()
    torch.cuda.set_device(0)
    amd.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    xb = amd.float_rand(nb * d, 1234).reshape(nb, d)
    xq = amd.float_rand(nq * d, 5678).reshape(nq, d)
    rf = amd.index_factory(d, f"IVF{nlist},PQ32,RFlat")
    rf.train(xb[:ntrain])
    rf.add(xb)
    base = rf.base_index
    base.nprobe = nprobe
    rf.sync_device()
    print(f"built in {time.time() - t0:.1f}s", flush=True)
    x_t = torch.from_numpy(xq).to(dev)
    ts = torch.cuda.Stream(device=dev)
    assert ts.cuda_stream != 0
    # ground truth: the flat storage itself, searched exhaustively
    Igt = np.empty((nq, k), np.int64)
    for q0 in range(0, nq, 2000):
        Igt[q0:q0 + 2000] = rf.refine_index.search(xq[q0:q0 + 2000], k)[1]
    ref_file = None
    try:
        from oracle import reflib
        if reflib.available():
            ref_file = os.path.join(tempfile.mkdtemp(), "refine_c3.faiss")
            amd.write_index(rf, ref_file)
    except Exception as e:  # no reference library here: the leg is "not measured"
        print("reference leg unavailable:", e, flush=True)
    legs = []
    for kf in (1, 4, 16):
        kb = k * kf
        rf.k_factor = kf
        Db = torch.empty((nq, kb), dtype=torch.float32, device=dev)
        Ib = torch.empty((nq, kb), dtype=torch.int64, device=dev)
        Dw = torch.empty((nq, k), dtype=torch.float32, device=dev)
        Iw = torch.empty((nq, k), dtype=torch.int64, device=dev)
        for _ in range(args.warmup):
            timed(base, x_t, kb, Db, Ib, ts, 1)
            timed(rf, x_t, k, Dw, Iw, ts, 1)
        half = max(1, args.steps // 2)
        b_ms, w_ms = [], []
        for _ in range(2):  # alternating blocks
            b_ms.append(timed(base, x_t, kb, Db, Ib, ts, half))
            w_ms.append(timed(rf, x_t, k, Dw, Iw, ts, half))
        amd.set_kernel_timing(True)
        rf.reset_kernel_times()
        timed(rf, x_t, k, Dw, Iw, ts, half)
        stages = {}
        for nm, ms, _ in rf.kernel_times():
            stages[nm] = stages.get(nm, 0.0) + ms / half
        amd.set_kernel_timing(False)
        rf.reset_kernel_times()
        refine_ms = stages.get("refine", float("nan"))
        model = nq * kb * (4 * d + 12)
        leg = {"k_factor": kf, "k_base": kb,
               "base_search_ms": float(np.mean(b_ms)), "base_search_ms_blocks": b_ms,
               "wrapper_search_ms": float(np.mean(w_ms)), "wrapper_search_ms_blocks": w_ms,
               "refine_stage_ms": refine_ms, "stage_ms_timed_pass": stages,
               "refine_byte_model": model,
               "refine_model_gbs": model / (refine_ms * 1e-3) / 1e9,
               "refine_model_frac_hbm_peak": model / (refine_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
               "recall10_base": recall_at_10(Ib.cpu().numpy()[:, :k], Igt),
               "recall10_wrapper": recall_at_10(Iw.cpu().numpy(), Igt),
               "reference_cpu_ms": None}
        if ref_file:
            with open(ref_file, "r+b") as f:  # k_factor: the file's last 4 bytes
                f.seek(-4, os.SEEK_END)
                f.write(struct.pack("<f", kf))
            ref = reflib.RefIndex(ref_file)
            ref.search(xq[:100], k, args.ref_threads)
            t1 = time.time()
            _, Ir = ref.search(xq, k, args.ref_threads)
            leg["reference_cpu_ms"] = (time.time() - t1) * 1e3
            leg["reference_cpu_threads"] = args.ref_threads
            leg["ids_equal_reference"] = bool(np.array_equal(Ir, Iw.cpu().numpy()))
            del ref
        print(json.dumps(leg), flush=True)
        legs.append(leg)
    if ref_file:
        os.remove(ref_file)
    out = {"shape": {"index": f"IVF{nlist},PQ32,RFlat", "d": d, "nb": nb, "nq": nq,
                     "nprobe": nprobe, "k": k, "steps": args.steps, "warmup": args.warmup},
           "hbm_peak_gbs": PEAK_HBM_GBS, "legs": legs,
           "device": torch.cuda.get_device_name(0)}
    txt = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
