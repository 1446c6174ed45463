#!/usr/bin/env python3
"""4-bit IVF-PQ on the c3 shape: IVF4096, d = 128, 1M float_rand vectors, 10k
device-resident queries, nprobe 32, k 10.

Three search_device steps are timed in one process, in alternating blocks,
with HIP events after a warm-up (as bench.py times its steps):
  lut    IVF4096,PQ32x4 on the default path, the LDS-table list scan
         (csrc/kernels_pq_lut.hip);
  exact  the same index with FAISS_AMD_PQ_SCAN=exact, the general exact scan
         (csrc/kernels_exact.hip);
  pq8    IVF4096,PQ32x8 (bench.py's c3 index) on the same build.
Also recorded: the stage timers of one timed pass of each, 10-recall@10 of each
against an exact IndexFlat, whether lut and exact agree bit for bit, the
reference's search of the PQ32x4 index file on 16 CPU threads (oracle/reflib.py,
when oracle/_ref is present) and whether its result equals ours, the byte MODEL
sum over probed rows of roundup(code_size, 4) and the lookup count rows * M
(models, not counter readings), the scan's candidate counters (the library's
FAISS_AMD_IVF_STATS line of one untimed search), and the kernels' registers,
LDS and occupancy as the compiler reports them (-Rpass-analysis=
kernel-resource-usage; --resources-only FILE collects them where hipcc is, with
no device, and --resources FILE merges them into the result).

Writes profiles/pq_nbits_c3.json (or --out) and prints it.

    python scripts/exp_pq_nbits.py [--steps 20] [--warmup 5] [--blocks 4]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


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


def kernel_resources():
    """{kernel: {VGPRs, ScratchSize, Occupancy, LDS Size}} of kernels_pq_lut.hip and
    of the k_ex_pq instantiations, from the compiler's remarks (no device)."""
    out = {}
    src = os.path.join(ROOT, "hnsw-ivf_amd", "csrc")
    for f in ("kernels_pq_lut.hip", "kernels_exact.hip"):
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC",
                                "-ffp-contract=off", "--offload-arch=gfx950",
                                "-Rpass-analysis=kernel-resource-usage", "-c",
                                os.path.join(src, f), "-o", os.path.join(tmp, "o.o")],
                               capture_output=True, text=True, check=True)
        cur = None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True,
                                      text=True).stdout.strip()
                m2 = re.search(r"(k_lut_\w+<\w+>|k_ex_pq<\w+, \d+>)", name)
                cur = m2.group(1) if m2 else None
                if cur:
                    out[cur] = {}
                continue
            m = re.search(r"remark: [^:]*?(VGPRs|ScratchSize \[bytes/lane\]|"
                          r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and cur:
                out[cur][m.group(1)] = int(m.group(2))
    return out


def set_scan(mode):
    if mode == "exact":
        os.environ["FAISS_AMD_PQ_SCAN"] = "exact"
    else:
        os.environ.pop("FAISS_AMD_PQ_SCAN", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--ref-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pq_nbits_c3.json"))
    ap.add_argument("--resources", default=None, help="kernel resource JSON to merge")
    ap.add_argument("--resources-only", default=None, metavar="FILE",
                    help="write the kernels' resource usage to FILE and stop (no device)")
    args = ap.parse_args()
    if args.resources_only:
        with open(args.resources_only, "w") as f:
            json.dump(kernel_resources(), f, indent=1)
        return
    d, nlist, nprobe, k, ntrain = 128, 4096, 32, 10, 200_000
    nb, nq = args.nb, args.nq
    amd = ge.load_package()
    torch.cuda.set_device(0)
    amd.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    xb = amd.float_rand(nb * d, 1234).reshape(nb, d)
    xq = amd.float_rand(nq * d, 5678).reshape(nq, d)
    idx = {}
    for name, desc in (("pq4", f"IVF{nlist},PQ32x4"), ("pq8", f"IVF{nlist},PQ32x8")):
        ix = amd.index_factory(d, desc)
        ix.train(xb[:ntrain])
        ix.add(xb)
        ix.nprobe = nprobe
        ix.sync_device()
        idx[name] = ix
        print(f"{desc} built, {time.time() - t0:.1f}s", flush=True)
    flat = amd.IndexFlatL2(d)
    flat.add(xb)
    Igt = np.empty((nq, k), np.int64)
    for q0 in range(0, nq, 2000):
        Igt[q0:q0 + 2000] = flat.search(xq[q0:q0 + 2000], k)[1]
    del flat
    x_t = torch.from_numpy(xq).to(dev)
    ts = torch.cuda.Stream(device=dev)
    D_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
    I_t = torch.empty((nq, k), dtype=torch.int64, device=dev)
    legs = (("lut", "pq4", "default"), ("exact", "pq4", "exact"), ("pq8", "pq8", "default"))
    res, ms = {}, {name: [] for name, _, _ in legs}
    for name, which, mode in legs:
        set_scan(mode)
        for _ in range(args.warmup):
            timed(idx[which], x_t, k, D_t, I_t, ts, 1)
        res[name] = (D_t.cpu().numpy().copy(), I_t.cpu().numpy().copy())
    per = max(1, args.steps // args.blocks)
    for _ in range(args.blocks):  # alternating blocks
        for name, which, mode in legs:
            set_scan(mode)
            ms[name].append(timed(idx[which], x_t, k, D_t, I_t, ts, per))
    stages = {}
    for name, which, mode in legs:
        set_scan(mode)
        amd.set_kernel_timing(True)
        idx[which].reset_kernel_times()
        timed(idx[which], x_t, k, D_t, I_t, ts, per)
        st = {}
        for nm, t, _ in idx[which].kernel_times():
            st[nm] = st.get(nm, 0.0) + t / per
        stages[name] = st
        amd.set_kernel_timing(False)
        idx[which].reset_kernel_times()
    set_scan("default")
    # the scan's candidate counters: the library prints them on stderr (fd 2)
    counters = None
    with tempfile.TemporaryFile() as tf:
        keep = os.dup(2)
        os.environ["FAISS_AMD_IVF_STATS"] = "1"
        try:
            os.dup2(tf.fileno(), 2)
            idx["pq4"].search(xq, k)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            os.environ.pop("FAISS_AMD_IVF_STATS", None)
        tf.seek(0)
        m = re.search(r"ivfpq lut scan: nq=(\d+) candidates/q=([0-9.]+) max=(\d+) "
                      r"overflow queries=(\d+) \(buffer (\d+)\)", tf.read().decode())
        if m:
            counters = {"nq": int(m.group(1)), "candidates_per_query": float(m.group(2)),
                        "max_candidates": int(m.group(3)), "overflow_queries": int(m.group(4)),
                        "buffer_entries": int(m.group(5)),
                        "scratch_bytes": int(m.group(1)) * (8 + 12 * int(m.group(5)))}
    # models of the probed rows (the coarse assignment of the timed queries)
    _, assign = idx["pq4"].quantizer.search(xq, nprobe)
    sizes = np.array([idx["pq4"].get_list_size(l) for l in range(nlist)], np.int64)
    rows = int(sizes[assign].sum())
    model = {}
    for which in ("pq4", "pq8"):
        cs = idx[which].code_size
        model[which] = {"code_size": cs, "probed_rows": rows,
                        "code_bytes": rows * ((cs + 3) // 4 * 4),
                        "lookups": rows * idx[which].pq_info()["M"],
                        "resident_bytes_per_row": cs + 16}
    out = {"shape": {"d": d, "nlist": nlist, "nb": nb, "nq": nq, "nprobe": nprobe, "k": k,
                     "steps_per_block": per, "blocks": args.blocks, "warmup": args.warmup},
           "device": torch.cuda.get_device_name(0),
           "ms_blocks": ms, "ms_mean": {n: float(np.mean(v)) for n, v in ms.items()},
           "pair_spread_ms": {n: float(np.max(v) - np.min(v)) for n, v in ms.items()},
           "stage_ms_timed_pass": stages,
           "recall10": {n: recall_at_10(res[n][1], Igt) for n in res},
           "lut_equals_exact": bool(np.array_equal(res["lut"][0], res["exact"][0]) and
                                    np.array_equal(res["lut"][1], res["exact"][1])),
           "model": model, "lut_counters": counters, "kernel_resources": None,
           "reference_cpu": None}
    if args.resources:
        out["kernel_resources"] = json.load(open(args.resources))
    try:
        from oracle import reflib
        if reflib.available():
            f = os.path.join(tempfile.mkdtemp(), "pq32x4_c3.faiss")
            amd.write_index(idx["pq4"], f)
            ref = reflib.RefIndex(f)
            ref.set_nprobe(nprobe)
            ref.search(xq[:100], k, args.ref_threads)
            t1 = time.time()
            Dr, Ir = ref.search(xq, k, args.ref_threads)
            out["reference_cpu"] = {"ms": (time.time() - t1) * 1e3, "threads": args.ref_threads,
                                    "recall10": recall_at_10(Ir, Igt),
                                    "ids_equal_ours": bool(np.array_equal(Ir, res["lut"][1])),
                                    "distances_equal_ours": bool(np.array_equal(Dr, res["lut"][0]))}
            del ref
            os.remove(f)
    except Exception as e:  # no reference library here: the leg is "not measured"
        print("reference leg unavailable:", e, flush=True)
    txt = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
