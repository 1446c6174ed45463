#!/usr/bin/env python3
"""Reference-run fixtures for IndexIVFScalarQuantizer (SQ8, SQfp16).

Writes tests/golden/ref_sq/<tag>.faiss (the reference's own write_index) and
tests/golden/ref_sq.npz (reference search / assign / encode results).  Runs
only where oracle/_ref/libfaissfull.so exists (the reference CPU library that
`make -C oracle/ref full` compiles), through the reff_* entry points it already
exports.  Searches run with one OpenMP thread, so IndexIVF::search treats the
batch as one slice; nq >= 20 makes the flat coarse quantizer take its BLAS form
(see oracle/ref/make_golden_full.py).

Inputs are ref_float_rand streams.  The query sets are stored; the training
set xt, the base set xb and the add set xa are stored as (rows, d, seed) plus a
SHA-256 of the bytes the reference consumed, because the raw arrays would not
fit the size limit of a committed file: the library's float_rand restates the
stream bit for bit, and the tests check the digest of what they regenerate.
In every index the last 10 % of xb are copies of its first rows, so equal
distances occur at the k-th place; xb is added with ids 3 i + 7.

    python scripts/make_golden_sq.py
"""
import ctypes as C
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTD = os.path.join(ROOT, "tests", "golden", "ref_sq")
OUT = os.path.join(ROOT, "tests", "golden", "ref_sq.npz")

L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissfull.so"), mode=C.RTLD_GLOBAL)
P, I64 = C.c_void_p, C.c_int64
L.reff_last_error.restype = C.c_char_p
L.reff_index_factory.restype = P
L.reff_index_factory.argtypes = [C.c_int, C.c_char_p, C.c_int]
L.reff_write_index.argtypes = [P, C.c_char_p]
L.reff_free.argtypes = [P]
L.reff_train.argtypes = [P, I64, P]
L.reff_add.argtypes = [P, I64, P, P]
L.reff_set_nprobe.argtypes = [P, I64]
L.reff_search.argtypes = [P, I64, P, I64, P, P]
L.reff_search_params.argtypes = [P, I64, P, I64, I64, I64, P, I64, P, P]
L.reff_quantizer_search.argtypes = [P, I64, P, I64, P, P]
L.reff_search_preassigned.argtypes = [P, I64, P, I64, I64, P, P, C.c_int, P, P]
L.reff_assign.argtypes = [P, I64, P, P]
L.reff_encode_vectors.argtypes = [P, I64, P, P, P]
L.reff_set_threads.argtypes = [C.c_int]

REFP = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissref.so"))
REFP.ref_float_rand.argtypes = [P, C.c_size_t, C.c_int64]

NQ = 32
NPROBES = (1, 4, None)  # None = nlist
KS = (1, 10, 100)

# tag, factory, metric_l2, d, nlist, nb, nt, code bytes per component
CASES = [
    ("sq8_l2_d64", "IVF32,SQ8", 1, 64, 32, 4000, 5000, 1),
    ("sq8_l2_d72", "IVF16,SQ8", 1, 72, 16, 2000, 3000, 1),
    ("sqfp16_l2_d64", "IVF32,SQfp16", 1, 64, 32, 3000, 5000, 2),
    ("sq8_ip_d64", "IVF32,SQ8", 0, 64, 32, 4000, 5000, 1),
    ("sq8_hnsw_d64", "IVF32_HNSW32,SQ8", 1, 64, 32, 4000, 5000, 1),
]


def p(a):
    return a.ctypes.data_as(P) if a is not None else None


def ok(rc):
    if rc != 0:
        raise RuntimeError(L.reff_last_error().decode())


def float_rand(n, d, seed):
    x = np.empty(n * d, np.float32)
    REFP.ref_float_rand(p(x), n * d, seed)
    return x.reshape(n, d)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def make_xb(nb, d, seed):
    xb = float_rand(nb, d, seed)
    dup = nb // 10
    xb[nb - dup:] = xb[:dup]
    return xb


def qsearch(h, x, nprobe):
    D = np.empty((x.shape[0], nprobe), np.float32)
    I = np.empty((x.shape[0], nprobe), np.int64)
    ok(L.reff_quantizer_search(h, x.shape[0], p(x), nprobe, p(D), p(I)))
    return D, I


def preassigned(h, x, k, Iq, Dq, store_pairs=0):
    n, nprobe = Iq.shape
    D = np.empty((n, k), np.float32)
    I = np.empty((n, k), np.int64)
    ok(L.reff_search_preassigned(h, n, p(x), k, nprobe, p(np.ascontiguousarray(Iq)),
                                 p(np.ascontiguousarray(Dq)), store_pairs, p(D), p(I)))
    return D, I


def main():
    os.makedirs(OUTD, exist_ok=True)
    fx = {}
    L.reff_set_threads(1)
    for ci, (tag, desc, ml2, d, nlist, nb, nt, bpc) in enumerate(CASES):
        seed = 7100 + 10 * ci
        h = L.reff_index_factory(d, desc.encode(), ml2)
        if not h:
            raise RuntimeError(L.reff_last_error().decode())
        xt = float_rand(nt, d, seed)
        xb = make_xb(nb, d, seed + 1)
        ids = np.arange(nb, dtype=np.int64) * 3 + 7
        ok(L.reff_train(h, nt, p(xt)))
        ok(L.reff_add(h, nb, p(xb), p(ids)))
        ok(L.reff_write_index(h, os.path.join(OUTD, tag + ".faiss").encode()))
        xq = float_rand(NQ, d, seed + 2)
        xq[-2:] = xb[:2]  # queries equal to (duplicated) base rows
        # [d, nlist, nb, nt, metric_l2, code_size, seed xt, seed xb, seed xq, seed xa, na]
        fx[f"{tag}_meta"] = np.array([d, nlist, nb, nt, ml2, d * bpc, seed, seed + 1, seed + 2,
                                      seed + 3, 500], np.int64)
        fx[f"{tag}_xq"] = xq
        fx[f"{tag}_xt_sha"], fx[f"{tag}_xb_sha"] = sha(xt), sha(xb)
        for npb in NPROBES:
            nprobe = npb or nlist
            Dq, Iq = qsearch(h, xq, nprobe)
            fx[f"{tag}_q{nprobe}_D"], fx[f"{tag}_q{nprobe}_I"] = Dq, Iq.astype(np.int32)
            for k in KS:
                D, I = preassigned(h, xq, k, Iq, Dq)
                fx[f"{tag}_pre_{nprobe}_{k}_D"] = D
                fx[f"{tag}_pre_{nprobe}_{k}_I"] = I.astype(np.int32)
        ok(L.reff_set_nprobe(h, 4))
        D = np.empty((NQ, 10), np.float32)
        I = np.empty((NQ, 10), np.int64)
        ok(L.reff_search(h, NQ, p(xq), 10, p(D), p(I)))
        fx[f"{tag}_full_4_10_D"], fx[f"{tag}_full_4_10_I"] = D, I.astype(np.int32)
        if tag in ("sq8_l2_d64", "sq8_ip_d64"):
            Dq, Iq = qsearch(h, xq, 4)
            D, I = preassigned(h, xq, 10, Iq, Dq, store_pairs=1)
            fx[f"{tag}_sp_D"], fx[f"{tag}_sp_I"] = D, I  # (list << 32 | offset: int64)
            sel = np.ascontiguousarray(ids[::2])
            D = np.empty((NQ, 10), np.float32)
            I = np.empty((NQ, 10), np.int64)
            ok(L.reff_search_params(h, NQ, p(xq), 10, 8, 300, p(sel), sel.size, p(D), p(I)))
            fx[f"{tag}_params_D"], fx[f"{tag}_params_I"] = D, I.astype(np.int32)
        if tag == "sq8_l2_d72":
            # nprobe = nlist, k = nb: every row's distance, in the heap's order
            xq20 = np.ascontiguousarray(xq[:20])
            Dq, Iq = qsearch(h, xq20, nlist)
            D, I = preassigned(h, xq20, nb, Iq, Dq)
            fx[f"{tag}_all_D"], fx[f"{tag}_all_I"] = D, I.astype(np.int32)
        xa = float_rand(500, d, seed + 3)
        la = np.empty(500, np.int64)
        ok(L.reff_assign(h, 500, p(xa), p(la)))
        codes = np.zeros((500, d * bpc), np.uint8)
        ok(L.reff_encode_vectors(h, 500, p(xa), p(la), p(codes)))
        fx[f"{tag}_xa_sha"] = sha(xa)
        fx[f"{tag}_xa_assign"], fx[f"{tag}_xa_codes"] = la.astype(np.int32), codes
        L.reff_free(h)
    np.savez_compressed(OUT, **fx)
    tot = os.path.getsize(OUT)
    print(f"{OUT}: {tot} bytes")
    for tag, *_ in CASES:
        f = os.path.join(OUTD, tag + ".faiss")
        print(f"{f}: {os.path.getsize(f)} bytes")
        tot += os.path.getsize(f)
    print(f"total {tot} bytes")


if __name__ == "__main__":
    main()
