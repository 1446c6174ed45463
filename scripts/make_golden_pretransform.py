#!/usr/bin/env python3
"""Reference-run fixtures for IndexPreTransform ("OPQ8_32,IVF16,PQ8" and
"PCA24,IVF16,Flat").

Writes tests/golden/ref_pretransform/<tag>.faiss and <tag>.npz.  Runs only
where oracle/_ref/libfaissfull.so exists (the reference CPU library that
`make -C oracle/ref full` compiles), through the reff_* entry points it
already exports: reff_index_factory, reff_train (which trains the OPQ / PCA
matrix: this library cannot), reff_add, reff_write_index, reff_search,
reff_set_threads(1).  nprobe stays at the sub-index's default of 1: the
wrapper hides it from reff_set_nprobe.

Inputs are ref_float_rand streams: NB rows of d = 40, 32 queries.  Recorded:
the reference's top 11 (the test compares 10 and needs the gap to the 11th).

The reference applies the transform with sgemm, whose summation order is not
this library's, so the test compares a query's ids only when every gap between
consecutive reference distances exceeds what the two roundings can move a
distance (gap_bound below, the test's formula).  At most 10 % of the queries
may be set aside that way; this script checks it on the reference's results
alone and tries the next seed until it holds (the seed used is recorded).

    python scripts/make_golden_pretransform.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTD = os.path.join(ROOT, "tests", "golden", "ref_pretransform")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pretransform_bound import comparable  # noqa: E402

L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissfull.so"), mode=C.RTLD_GLOBAL)
P, I64 = C.c_void_p, C.c_int64
L.reff_last_error.restype = C.c_char_p
L.reff_index_factory.restype = P
L.reff_index_factory.argtypes = [C.c_int, C.c_char_p, C.c_int]
L.reff_write_index.argtypes = [P, C.c_char_p]
L.reff_free.argtypes = [P]
L.reff_train.argtypes = [P, I64, P]
L.reff_add.argtypes = [P, I64, P, P]
L.reff_search.argtypes = [P, I64, P, I64, P, P]
L.reff_set_threads.argtypes = [C.c_int]

REFP = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissref.so"))
REFP.ref_float_rand.argtypes = [P, C.c_size_t, C.c_int64]

D, NB, NQ, K = 40, 2000, 32, 11
CASES = [("opq8_32_ivf16_pq8", "OPQ8_32,IVF16,PQ8"), ("pca24_ivf16_flat", "PCA24,IVF16,Flat")]


def p(a):
    return a.ctypes.data_as(P)


def ok(rc):
    if rc != 0:
        raise RuntimeError(L.reff_last_error().decode())


def float_rand(n, d, seed):
    x = np.empty(n * d, np.float32)
    REFP.ref_float_rand(p(x), n * d, seed)
    return x.reshape(n, d)


def read_transform(path):
    """(A [d_out][d_in], b [d_out]) of the file's one transform, through this
    library's reader (the gap bound needs them)."""
    import __graft_entry__ as ge
    amd = ge.load_package()
    t, = amd.read_index(path).chain
    A = t.A.reshape(t.d_out, t.d_in)
    return A, (t.b if t.have_bias else np.zeros(t.d_out, np.float32))


def main():
    sys.path.insert(0, ROOT)
    os.makedirs(OUTD, exist_ok=True)
    L.reff_set_threads(1)
    for tag, desc in CASES:
        for seed in range(100, 120):
            xb, xq = float_rand(NB, D, seed), float_rand(NQ, D, seed + 1000)
            h = L.reff_index_factory(D, desc.encode(), 1)
            assert h, L.reff_last_error().decode()
            ok(L.reff_train(h, NB, p(xb)))
            ok(L.reff_add(h, NB, p(xb), None))
            Dr = np.empty((NQ, K), np.float32)
            Ir = np.empty((NQ, K), np.int64)
            ok(L.reff_search(h, NQ, p(xq), K, p(Dr), p(Ir)))
            path = os.path.join(OUTD, tag + ".faiss")
            ok(L.reff_write_index(h, path.encode()))
            L.reff_free(h)
            A, b = read_transform(path)
            keep = comparable(xq, A, b, Dr)
            print(f"{tag} seed {seed}: {int((~keep).sum())}/{NQ} queries set aside")
            if (~keep).sum() <= NQ // 10 and (Ir >= 0).all():
                break
        else:
            raise SystemExit(f"{tag}: no seed keeps 90 % of the queries comparable")
        np.savez(os.path.join(OUTD, tag + ".npz"), D=Dr, I=Ir,
                 meta=np.array([seed, NB, NQ, K], np.int64))
        print(f"{tag}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
