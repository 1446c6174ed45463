#!/usr/bin/env python3
"""Reference-run fixtures for IndexIVF::remove_ids / update_vectors, the direct
maps and the reconstruct family (reconstruct, reconstruct_n,
search_and_reconstruct).

Compiles scripts/mutation_driver.cpp against the reference's public headers
and the objects `make -C oracle/ref full` leaves in oracle/_ref/fobj (all but
ref_full_driver.o), with that Makefile's MKL link line, into
oracle/_ref/mutation_driver, and runs it on one OpenMP thread.  Writes
tests/golden/ref_mutation.npz (the SQ8 decode table), one
tests/golden/ref_mutation/<tag>.npz per index and
tests/golden/ref_mutation/*.faiss (the reference's own write_index).  Run
once; the tests only read the output.

Indexes (IVF16, NB rows of numpy default_rng(seed) standard normals, the last
NB / 10 rows copies of the first, sequential ids):
  flat     IVF16,Flat      d 32  L2
  pq8      IVF16,PQ8       d 32  L2   (+ the files with an Array / Hashtable map)
  pq12x5   IVF16,PQ12x5    d 24  L2   (60-bit codes: fields straddle bytes)
  sq8      IVF16,SQ8       d 32  L2   by residual
  sqfp16   IVF16,SQfp16    d 32  inner product
Queries: 20 random rows + 12 base rows.

An index's npz holds the driver's records under <tag>_<record> (see the head
of scripts/mutation_driver.cpp), with these reductions to keep the files small:
ids as int32; each list's codes after a mutation as one sha256 per list
(<record>_codes_sha [nlist][32]).  The three map-less removals keep their
results at k = 1, 10 and 100; the Hashtable removal and update_vectors, for
which no k is asked, keep k = 1 and 10.

The generator asserts, from the reference's own output, that every removal
changes the k = 10 ids of at least half the queries, that some list's order
after a removal differs from the order of its survivors, and that the SQ8
decode table (sq_decode: all 256 codes x 8 (vmin, vdiff) pairs) tells the
candidate formulas apart: it names the one that reproduces every value in
sq_formula.

    python scripts/make_golden_mutation.py
"""
import glob
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REF", "/root/reference")
OREF = os.path.join(ROOT, "oracle", "_ref")
DRIVER = os.path.join(OREF, "mutation_driver")
GOLD = os.path.join(ROOT, "tests", "golden")
OUTD = os.path.join(GOLD, "ref_mutation")
OUT = os.path.join(GOLD, "ref_mutation.npz")

NB, NQ, SEED0 = 2000, 32, 7300
INDEXES = (  # tag, factory, metric, d
    ("flat", "IVF16,Flat", "l2", 32),
    ("pq8", "IVF16,PQ8", "l2", 32),
    ("pq12x5", "IVF16,PQ12x5", "l2", 24),
    ("sq8", "IVF16,SQ8", "l2", 32),
    ("sqfp16", "IVF16,SQfp16", "ip", 32),
)
REMOVALS = ("range", "batch", "array", "hash")


def compile_driver():
    objs = [o for o in glob.glob(os.path.join(OREF, "fobj", "**", "*.o"), recursive=True)
            if os.path.basename(o) != "ref_full_driver.o"]
    assert objs, "run `make -C oracle/ref full` first"
    cmd = ["g++", "-O2", "-std=c++17", "-fopenmp", "-mavx2", "-mfma", "-mf16c", "-mpopcnt",
           "-DFINTEGER=int", "-I" + REF, "-w",
           os.path.join(ROOT, "scripts", "mutation_driver.cpp"), *objs, "-o", DRIVER,
           "-L" + os.path.join(OREF, "mkl"), "-lmkl_intel_lp64", "-lmkl_gnu_thread", "-lmkl_core",
           "-lgomp", "-lpthread", "-lm", "-Wl,-rpath,$ORIGIN/mkl"]
    subprocess.run(cmd, check=True)


def read_records(fn):
    raw = open(fn, "rb").read()
    out, p = {}, 0
    types = {0: np.float32, 1: np.int64, 2: np.uint8, 3: np.uint32}
    while p < len(raw):
        (ln,) = struct.unpack_from("<I", raw, p)
        name = raw[p + 4:p + 4 + ln].decode()
        p += 4 + ln
        t, nd = struct.unpack_from("<BI", raw, p)
        p += 5
        dims = struct.unpack_from(f"<{nd}Q", raw, p)
        p += 8 * nd
        dt = np.dtype(types[t])
        n = int(np.prod(dims)) if nd else 1
        out[name] = np.frombuffer(raw, dt, n, offset=p).reshape(dims).copy()
        p += n * dt.itemsize
    return out


def list_sha(sizes, codes, code_size):
    """[nlist][32] uint8: sha256 of each list's code bytes."""
    out, p = [], 0
    for n in sizes:
        nb = int(n) * code_size
        out.append(np.frombuffer(hashlib.sha256(codes[p:p + nb].tobytes()).digest(), np.uint8))
        p += nb
    assert p == len(codes)
    return np.stack(out)


def sq_candidates(vmin, vdiff):
    """name -> [256][8] float32 of the candidate decode formulas, every
    operation rounded to fp32 (numpy float32 arithmetic; the fused forms in
    float64, exact for these products, rounded once)."""
    c = np.arange(256, dtype=np.float32)[:, None]
    xi_div = (c + np.float32(0.5)) / np.float32(255.0)
    k1, k2 = np.float32(1.0) / np.float32(255.0), np.float32(0.5) / np.float32(255.0)
    xi_fma = (c.astype(np.float64) * np.float64(k1) + np.float64(k2)).astype(np.float32)

    def fused(xi):
        return (xi.astype(np.float64) * vdiff.astype(np.float64)
                + vmin.astype(np.float64)).astype(np.float32)

    def plain(xi):
        return (xi * vdiff).astype(np.float32) + vmin

    return {"div_fma": fused(xi_div), "div_plain": plain(xi_div),
            "scan_fma": fused(xi_fma), "scan_plain": plain(xi_fma)}


def sq_table(fx):
    with tempfile.TemporaryDirectory() as tmp:
        rec = os.path.join(tmp, "sq.rec")
        subprocess.run([DRIVER, "sqtable", rec], check=True)
        r = read_records(rec)
    got = r["sq_decode"]
    cands = {k: v.view(np.uint32) for k, v in sq_candidates(r["sq_vmin"], r["sq_vdiff"]).items()}
    hits = [k for k, v in cands.items() if np.array_equal(v, got)]
    diff = {k: int((v != got).sum()) for k, v in cands.items()}
    print("SQ8 decode: values differing from the reference per candidate:", diff)
    assert len(hits) == 1, f"the table does not single out one formula: {hits}"
    assert any(n > 0 for n in diff.values()), "no stored value tells the formulas apart"
    fx["sq_vmin"], fx["sq_vdiff"], fx["sq_decode"] = r["sq_vmin"], r["sq_vdiff"], got
    fx["sq_formula"] = np.array(hits[0])


def make_index(fx, tag, factory, metric, d, seed):
    rng = np.random.default_rng(seed)
    xb = rng.standard_normal((NB, d), dtype=np.float32)
    xb[NB - NB // 10:] = xb[:NB // 10]
    xq = rng.standard_normal((NQ, d), dtype=np.float32)
    xq[20:] = xb[rng.choice(NB, NQ - 20, replace=False)] + np.float32(0.01)
    base = os.path.join(OUTD, tag + ".faiss")
    with tempfile.TemporaryDirectory() as tmp:
        bf, qf, rec = (os.path.join(tmp, n) for n in ("xb.f32", "xq.f32", "out.rec"))
        xb.tofile(bf)
        xq.tofile(qf)
        cmd = [DRIVER, "index", factory, metric, str(d), str(NB), bf, str(NQ), qf, base, rec]
        if tag == "pq8":
            cmd += [os.path.join(OUTD, "pq8_array.faiss"), os.path.join(OUTD, "pq8_hash.faiss")]
        subprocess.run(cmd, check=True)
        r = read_records(rec)
    code_size = len(r["base_codes"]) // NB
    # ---- what the tests rely on, from the reference's own output
    changed, reordered = {}, False
    for s in REMOVALS:
        changed[s] = float((r[f"rm_{s}_k10_I"] != r["base_k10_I"]).any(axis=1).mean())
        p = q = 0
        for l, (n0, n1) in enumerate(zip(r["base_sizes"], r[f"rm_{s}_sizes"])):
            before = r["base_ids"][p:p + n0]
            after = r[f"rm_{s}_ids"][q:q + n1]
            surv = before[np.isin(before, after)]
            reordered |= not np.array_equal(surv, after)
            p, q = p + n0, q + n1
    ok = all(v >= 0.5 for v in changed.values()) and reordered
    print(f"{tag} seed {seed}: queries changed at k=10 {changed}; a list reordered: {reordered}; "
          f"pad k {int(r['pad_k'][0])}; {os.path.getsize(base)} bytes")
    if not ok:
        return False
    assert r["array_refusal"].size and r["hash_refusal"].size
    assert (r["pad_I"] == -1).any() and (r["pad_R"] == 0xFFFFFFFF).any()
    # ---- pack
    fx[f"{tag}_seed"] = np.array([seed, NB, d, code_size], np.int64)
    fx[f"{tag}_xq"] = xq
    for name, a in r.items():
        if name.endswith("_codes"):
            sizes = r[name[:-6] + "_sizes"]
            fx[f"{tag}_{name}_sha"] = list_sha(sizes, a, code_size)
        elif "_k100_" in name and name.split("_k100_")[0] not in (
                "rm_range", "rm_batch", "rm_array"):
            continue
        elif name.startswith("base_k"):
            continue  # (the assertions above only)
        elif a.dtype == np.int64 and not name.endswith("_map") and not name.endswith("_sel"):
            assert np.abs(a).max(initial=0) < 2 ** 31
            fx[f"{tag}_{name}"] = a.astype(np.int32)
        else:
            fx[f"{tag}_{name}"] = a
    return True


def main():
    os.makedirs(OUTD, exist_ok=True)
    compile_driver()
    fx = {}
    sq_table(fx)
    np.savez_compressed(OUT, **fx)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    for tag, factory, metric, d in INDEXES:
        fx = {}
        for seed in range(SEED0, SEED0 + 20):
            if make_index(fx, tag, factory, metric, d, seed):
                break
        else:
            sys.exit(f"{tag}: no seed meets the generator's assertions")
        np.savez_compressed(os.path.join(OUTD, tag + ".npz"), **fx)
    for f in sorted(os.listdir(OUTD)):
        print(f"  {f}: {os.path.getsize(os.path.join(OUTD, f))} bytes")


if __name__ == "__main__":
    main()
