#!/usr/bin/env python3
"""Reference-run fixtures for METRIC_INNER_PRODUCT on IndexHNSWFlat, alone and
as the coarse quantizer of IVF-Flat / IVF-PQ.

Uses scripts/hnsw_params_driver.cpp (compiled as make_golden_hnsw_params.py
compiles it, against the objects `make -C oracle/ref full` leaves in
oracle/_ref/fobj) on one OpenMP thread: `build ... ip` makes, trains and fills
an index with the reference's own index_factory / train / add / write_index,
`run` searches it (the index file carries the metric), `coarse` searches an
IVF index's quantizer on its own.  Writes tests/golden/ref_hnsw_ip.npz,
tests/golden/ref_hnsw_ip/*.faiss and (the cases of hnsw8_ip_d16, which would
take the first file past the size limit)
tests/golden/ref_hnsw_ip/hnsw8_ip_d16.npz.  Every job goes through the driver,
the default-mode ones too (not the reff_* entry points of libfaissfull.so,
which hold the same reference objects).  Run once; the tests only read the
output.

Indexes (rows: numpy default_rng(seed) standard normals, each row scaled by a
factor drawn uniformly from [0.25, 4], so that the largest inner product is
not the nearest row):
  hnsw16_ip_d24            HNSW16,Flat, d 24 (ld no multiple of 8), 1500 rows,
                           the last 200 copies of the first 200, row 750 zero
  hnsw8_ip_d16             HNSW8,Flat, d 16, 900 rows, the last 300 copies
  ivf64_hnsw8_ip_flat_d32  IVF64_HNSW8,Flat, d 32, 2000 rows
  ivf64_hnsw8_ip_pq8_d32   IVF64_HNSW8,PQ8, d 32, the same rows
Queries: 40 random rows + 24 base rows per index.

Standalone jobs: efSearch {1, 16, 64, 200, 5000} x k {1, 10, 100} in the
default mode, with check_relative_distance false (A) and with bounded_queue
false (B); the five selectors of make_golden_hnsw_params.py at ef 64, k 10.
IVF jobs: nprobe {1, 8, 64} x quantizer efSearch {16, 64} — the quantizer's
own (distances, ids) and the index's results — and one quantizer_params job
with check_relative_distance false.  Every search records hnsw_stats.

The generator asserts, from the reference's own output: for at least half of
hnsw16_ip_d24's queries the top-1 id differs from that of an L2 HNSW16 over
the same rows (an L2 kernel cannot pass); every distance D of a filled slot
satisfies D == -(-D) bitwise (the reference negates its -<q, y> on the way
out; documented, trivially true); `three` and `empty` pad with (-FLT_MAX, -1);
some duplicate-row case has a tie at the k-th slot.  It tries seeds from SEED0
until this holds.

    python scripts/make_golden_hnsw_ip.py
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_hnsw_params import (DRIVER, EFS, GOLD, KS, compile_driver, run_jobs,  # noqa: E402
                                     sel_specs)

OUTD = os.path.join(GOLD, "ref_hnsw_ip")
OUT = os.path.join(GOLD, "ref_hnsw_ip.npz")
OUT_H8 = os.path.join(OUTD, "hnsw8_ip_d16.npz")
SEED0 = 5200
LIMIT = 480 * 1024
FLT_MAX = np.float32(3.4028234663852886e38)
STANDALONE = {"h16": ("hnsw16_ip_d24", "HNSW16", 24, 1500, 200, 750),
              "h8": ("hnsw8_ip_d16", "HNSW8", 16, 900, 300, -1)}
IVF = {"ivfflat": ("ivf64_hnsw8_ip_flat_d32", "IVF64_HNSW8,Flat"),
       "ivfpq": ("ivf64_hnsw8_ip_pq8_d32", "IVF64_HNSW8,PQ8")}
IVF_D, IVF_NB = 32, 2000
NPROBES, QEFS = (1, 8, 64), (16, 64)


def rows(rng, n, d):
    x = rng.standard_normal((n, d), dtype=np.float32)
    return (x * rng.uniform(0.25, 4.0, (n, 1)).astype(np.float32)).astype(np.float32)


def queries(rng, xb):
    xq = rows(rng, 64, xb.shape[1])
    xq[40:] = xb[rng.choice(xb.shape[0], 24, replace=False)]
    return xq


def build(desc, xb, fn, metric):
    with tempfile.TemporaryDirectory() as tmp:
        bf = os.path.join(tmp, "xb.f32")
        xb.tofile(bf)
        subprocess.run([DRIVER, "build", desc, str(xb.shape[1]), str(xb.shape[0]), bf, fn, metric],
                       check=True)


def standalone_jobs(n):
    jobs = []
    for ef in EFS:
        for k in KS:
            jobs.append((f"def_ef{ef}_k{k}", k, "params", ef, 1, 1, "none", 0))
            jobs.append((f"A_ef{ef}_k{k}", k, "params", ef, 0, 1, "none", 0))
            jobs.append((f"B_ef{ef}_k{k}", k, "params", ef, 1, 0, "none", 0))
    for sn, spec in sel_specs(n).items():
        jobs.append((f"sel_{sn}", 10, "params", 64, 1, 1, spec, 0))
    return jobs


def ivf_jobs():
    jobs = [(f"np{np_}_ef{ef}", 10, "index", ef, 1, 1, "none", np_)
            for np_ in NPROBES for ef in QEFS]
    jobs.append(("qpA_np8", 10, "params", 64, 0, 1, "none", 8))
    return jobs


def coarse(fn, xq, ef, k):
    nq, d = xq.shape
    with tempfile.TemporaryDirectory() as tmp:
        xf, of = os.path.join(tmp, "xq.f32"), os.path.join(tmp, "o.bin")
        xq.tofile(xf)
        subprocess.run([DRIVER, "coarse", fn, str(d), str(nq), xf, str(ef), str(k), of], check=True)
        raw = open(of, "rb").read()
    assert len(raw) == nq * k * 12
    return (np.frombuffer(raw, np.float32, nq * k).reshape(nq, k).copy(),
            np.frombuffer(raw, np.int64, nq * k, offset=nq * k * 4).reshape(nq, k).copy())


def check_convention(res):
    for name, (D, I, _) in res.items():
        filled = I >= 0
        assert (D[~filled] == -FLT_MAX).all(), name  # padding: -(FLT_MAX)
        assert np.array_equal((-(-D)).view(np.uint32), D.view(np.uint32)), name
        assert (np.diff(D, axis=1) <= 0).all(), name  # largest first
    assert (res["sel_empty"][1] == -1).all() and (res["sel_three"][1][:, 3:] == -1).all()


def kth_tie(res):
    for name, (D, I, _) in res.items():
        k = D.shape[1]
        if k >= 2 and ((D[:, k - 1] == D[:, k - 2]) & (I[:, k - 1] >= 0)).any():
            return name
    return None


def digest(D):
    """sha256 of the distances' bytes (row-major float32), as 32 uint8."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(D, np.float32).tobytes()).digest(),
                         np.uint8)


def pack(fx, tag, xq, jobs, res):
    """Ids as int16 (every index has fewer than 2^15 rows).  A k = 100 job
    keeps the sha256 of its distances instead of the 25 KB array (45 such
    arrays would take the file past the size limit of a committed fixture):
    the tests hash what they get, which holds them to the same bits."""
    fx[f"{tag}_xq"] = xq
    fx[f"{tag}_jobs"] = np.array([" ".join(str(v) for v in j) for j in jobs])
    for j in jobs:
        D, I, st = res[j[0]]
        assert I.max() < 2 ** 15 and I.min() >= -1
        fx[f"{tag}_{j[0]}_I"] = I.astype(np.int16)
        fx[f"{tag}_{j[0]}_st"] = st
        if j[1] >= 100:
            fx[f"{tag}_{j[0]}_Dsha"] = digest(D)
        else:
            fx[f"{tag}_{j[0]}_D"] = D


def main():
    os.makedirs(OUTD, exist_ok=True)
    compile_driver()
    for seed in range(SEED0, SEED0 + 20):
        rng = np.random.default_rng(seed)
        fx, ok, ties = {}, True, []
        for tag, (name, desc, d, nb, ndup, zero) in STANDALONE.items():
            xb = rows(rng, nb, d)
            xb[nb - ndup:] = xb[:ndup]
            if zero >= 0:
                xb[zero] = 0
            xq = queries(rng, xb)
            fn = os.path.join(OUTD, name + ".faiss")
            build(desc, xb, fn, "ip")
            jobs = standalone_jobs(nb)
            res = run_jobs(fn, xq, jobs)
            check_convention(res)
            ties.append(kth_tie(res))
            if tag == "h16":
                with tempfile.TemporaryDirectory() as tmp:
                    f2 = os.path.join(tmp, "l2.faiss")
                    build(desc, xb, f2, "l2")
                    l2 = run_jobs(f2, xq, [("def_ef200_k1", 1, "params", 200, 1, 1, "none", 0)])
                frac = float((l2["def_ef200_k1"][1][:, 0] != res["def_ef200_k1"][1][:, 0]).mean())
                print(f"seed {seed}: top-1 differs from the L2 index for {frac:.2f} of the queries")
                ok = ok and frac >= 0.5
            ok = ok and os.path.getsize(fn) <= LIMIT
            pack(fx, tag, xq, jobs, res)
        print(f"seed {seed}: k-th slot ties in {ties}")
        if ok and any(ties):
            break
    else:
        sys.exit("no seed meets the assertions")
    xb = rows(rng, IVF_NB, IVF_D)
    xq = queries(rng, xb)
    for tag, (name, desc) in IVF.items():
        fn = os.path.join(OUTD, name + ".faiss")
        build(desc, xb, fn, "ip")
        assert os.path.getsize(fn) <= LIMIT, (fn, os.path.getsize(fn))
        jobs = ivf_jobs()
        res = run_jobs(fn, xq, jobs)
        pack(fx, tag, xq, jobs, res)
        for np_ in NPROBES:
            for ef in QEFS:
                Dq, Iq = coarse(fn, xq, ef, np_)
                assert (np.diff(Dq, axis=1) <= 0).all()
                fx[f"{tag}_coarse_np{np_}_ef{ef}_D"] = Dq
                fx[f"{tag}_coarse_np{np_}_ef{ef}_I"] = Iq.astype(np.int16)
    fx["seed"] = np.array([seed], np.int64)
    # (one file would be past the size limit: hnsw8_ip_d16's cases go beside its index)
    h8 = {k: fx.pop(k) for k in [k for k in fx if k.startswith("h8_")]}
    for fn, part in ((OUT, fx), (OUT_H8, h8)):
        np.savez_compressed(fn, **part)
        print(f"{fn}: {os.path.getsize(fn)} bytes")
        assert os.path.getsize(fn) <= LIMIT
    for f in sorted(os.listdir(OUTD)):
        print(f, os.path.getsize(os.path.join(OUTD, f)))


if __name__ == "__main__":
    main()
