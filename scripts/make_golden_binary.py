#!/usr/bin/env python3
"""Reference-run fixtures for the binary indexes (file tags IBxF, IBwF).

Writes tests/golden/ref_binary/{flat,ivf}.faiss (the reference's own bytes)
and ref_binary.npz: the inputs and the reference's D, I for every recorded
configuration.  Runs only where `make -C oracle/ref full` has compiled the
reference objects; compiles scripts/binary_driver.cpp against them.

d = 16 with 300 rows: 17 distinct distances, so nearly every k boundary falls
inside a tie group.  The IVF ids are a shuffled permutation, and the script
checks (with tests/binary_model.py's arrival order) that some query's ids do
not ascend along its arrival order.

    python scripts/make_golden_binary.py
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import binary_model as bm  # noqa: E402
from make_golden_hnsw_params import OREF, REF  # noqa: E402  (the reference tree and its objects)

DRIVER = os.path.join(OREF, "binary_driver")
OUTD = os.path.join(ROOT, "tests", "golden", "ref_binary")

D, NB, NQ, K, NLIST = 16, 300, 12, 10, 8
# tag -> (index, use_heap, nprobe, max_codes)
CONFIGS = {"flat_heap": ("flat", 1, 0, 0), "flat_count": ("flat", 0, 0, 0),
           "ivf_heap": ("ivf", 1, 3, 0), "ivf_count": ("ivf", 0, 3, 0),
           "ivf_heap_mc64": ("ivf", 1, 5, 64), "ivf_count_mc64": ("ivf", 0, 5, 64)}


def compile_driver():
    objs = [o for o in glob.glob(os.path.join(OREF, "fobj", "**", "*.o"), recursive=True)
            if os.path.basename(o) != "ref_full_driver.o"]
    assert objs, "run `make -C oracle/ref full` first"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-mavx2", "-mfma", "-mf16c",
                    "-mpopcnt", "-DFINTEGER=int", "-I" + REF, "-w",
                    os.path.join(ROOT, "scripts", "binary_driver.cpp"), *objs, "-o", DRIVER,
                    "-L" + os.path.join(OREF, "mkl"), "-lmkl_intel_lp64", "-lmkl_gnu_thread",
                    "-lmkl_core", "-lgomp", "-lpthread", "-lm", "-Wl,-rpath,$ORIGIN/mkl"],
                   check=True)


def main():
    compile_driver()
    os.makedirs(OUTD, exist_ok=True)
    rng = np.random.default_rng(9100)
    cs = D // 8
    xb = rng.integers(0, 256, (NB, cs), dtype=np.uint8)
    xq = rng.integers(0, 256, (NQ, cs), dtype=np.uint8)
    cent = rng.integers(0, 256, (NLIST, cs), dtype=np.uint8)
    ids = rng.permutation(NB).astype(np.int64) + 1000
    out = dict(xb=xb, xq=xq, cent=cent, ids=ids, k=np.int64(K))
    with tempfile.TemporaryDirectory() as t:
        p = lambda n: os.path.join(t, n)  # noqa: E731
        for name, a in (("xb", xb), ("xq", xq), ("cent", cent), ("ids", ids)):
            a.tofile(p(name))
        files = {"flat": os.path.join(OUTD, "flat.faiss"), "ivf": os.path.join(OUTD, "ivf.faiss")}
        subprocess.run([DRIVER, "flat", str(D), str(NB), p("xb"), files["flat"]], check=True)
        subprocess.run([DRIVER, "ivf", str(D), str(NB), p("xb"), p("ids"), str(NLIST), p("cent"),
                        files["ivf"]], check=True)
        for tag, (which, heap, nprobe, mc) in CONFIGS.items():
            subprocess.run([DRIVER, "search", files[which], str(NQ), p("xq"), str(K), str(heap),
                            str(nprobe), str(mc), p("D"), p("I")], check=True)
            out[tag + "_D"] = np.fromfile(p("D"), np.int32).reshape(NQ, K)
            out[tag + "_I"] = np.fromfile(p("I"), np.int64).reshape(NQ, K)
            out[tag + "_cfg"] = np.array([heap, nprobe, mc], np.int64)
            Dr = out[tag + "_D"]
            print(f"{tag}: {int((Dr[:, 1:] == Dr[:, :-1]).sum())} equal neighbours in D")
    model = bm.IVFModel(cent, xb, ids)
    desc = [bool((np.diff(ids[model.arrivals(q, 3)]) < 0).any()) for q in xq]
    assert any(desc), "no query with ids descending along the arrival order"
    print(f"{sum(desc)}/{NQ} queries have ids that do not ascend along the arrival order")
    np.savez(os.path.join(OUTD, "ref_binary.npz"), **out)


if __name__ == "__main__":
    main()
