#!/usr/bin/env python3
"""Reference-run fixtures for the 8-bit IVF-PQ geometries of the MFMA filter
that tests/golden/ref_full does not hold: M32 d64, M12 d96, M64 d128, M16 d128.

Writes tests/golden/ref_pq_filter/<tag>.faiss (the reference's own
write_index) and tests/golden/ref_pq_filter.npz (the reference's search
results).  Runs only where oracle/_ref/libfaissfull.so exists, through the
reff_* entry points it already exports, with one OpenMP thread throughout.

Per tag (tests/pq_filter_data.py ref_inputs): `IVF16,PQ<M>`, L2, by residual,
trained by the reference on 6000 float_rand rows; 2000 base rows (1600
distinct, 16 vectors 25 times each) added with permuted ids; 64 queries, half
of them copies of the repeated vectors.  Recorded: the index's fields and
list digest, the quantizer's keys and distances at nprobe 5, 8 and 16,
search_preassigned for precomputed tables 1 and 0 at (nprobe, k) = (16, 1),
(16, 10), (16, 20), (5, 10), and one IndexIVF::search with
SearchParametersIVF(nprobe 8, max_codes 300, IDSelectorBatch of ~40 % of the
ids).  The files are reference outputs (data); no reference text is copied.

    python scripts/make_golden_pq_filter.py
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import pq_filter_data as pf  # noqa: E402

OUTD = os.path.join(ROOT, "tests", "golden", "ref_pq_filter")
OUT = os.path.join(ROOT, "tests", "golden", "ref_pq_filter.npz")

L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissfull.so"), mode=C.RTLD_GLOBAL)
P, I64 = C.c_void_p, C.c_int64
L.reff_last_error.restype = C.c_char_p
L.reff_index_factory.restype = P
L.reff_index_factory.argtypes = [C.c_int, C.c_char_p, C.c_int]
L.reff_write_index.argtypes = [P, C.c_char_p]
L.reff_free.argtypes = [P]
L.reff_train.argtypes = [P, I64, P]
L.reff_add.argtypes = [P, I64, P, P]
L.reff_info.argtypes = [P, P]
L.reff_ivfpq_set_table.argtypes = [P, C.c_int]
L.reff_search_params.argtypes = [P, I64, P, I64, I64, I64, P, I64, P, P]
L.reff_quantizer_search.argtypes = [P, I64, P, I64, P, P]
L.reff_search_preassigned.argtypes = [P, I64, P, I64, I64, P, P, C.c_int, P, P]
L.reff_list_size.restype = I64
L.reff_list_size.argtypes = [P, I64]
L.reff_list_copy.argtypes = [P, I64, P, P]
L.reff_set_threads.argtypes = [C.c_int]


def p(a):
    return a.ctypes.data_as(P) if a is not None else None


def ok(rc):
    if rc != 0:
        raise RuntimeError(L.reff_last_error().decode())


def qsearch(h, x, nprobe):
    D = np.empty((x.shape[0], nprobe), np.float32)
    I = np.empty((x.shape[0], nprobe), np.int64)
    ok(L.reff_quantizer_search(h, x.shape[0], p(x), nprobe, p(D), p(I)))
    return D, I


def preassigned(h, x, k, Iq, Dq):
    n, nprobe = Iq.shape
    D = np.empty((n, k), np.float32)
    I = np.empty((n, k), np.int64)
    ok(L.reff_search_preassigned(h, n, p(x), k, nprobe, p(np.ascontiguousarray(Iq)),
                                 p(np.ascontiguousarray(Dq)), 0, p(D), p(I)))
    return D, I


def lists_digest(h, nlist, code_size):
    sizes = np.array([L.reff_list_size(h, l) for l in range(nlist)], np.int64)
    sha = hashlib.sha256()
    for l in range(nlist):
        n = int(sizes[l])
        codes = np.empty(max(n * code_size, 1), np.uint8)
        ids = np.empty(max(n, 1), np.int64)
        ok(L.reff_list_copy(h, l, p(codes), p(ids)))
        sha.update(codes[: n * code_size].tobytes())
        sha.update(ids[:n].tobytes())
    return sizes, np.frombuffer(sha.digest(), np.uint8)


def main():
    os.makedirs(OUTD, exist_ok=True)
    float_rand = ge.load_oracle().float_rand
    L.reff_set_threads(1)
    fx = {}
    for tag in pf.REF_TAGS:
        c = pf.ref_inputs(float_rand, tag)
        d, M, xq = c["d"], c["M"], c["xq"]
        h = L.reff_index_factory(d, f"IVF{pf.REF_NLIST},PQ{M}".encode(), 1)
        if not h:
            raise RuntimeError(L.reff_last_error().decode())
        ok(L.reff_train(h, pf.REF_NT, p(c["xt"])))
        ok(L.reff_add(h, pf.REF_NB, p(c["xb"]), p(c["ids"])))
        ok(L.reff_write_index(h, os.path.join(OUTD, tag + ".faiss").encode()))
        inf = np.zeros(10, np.int64)
        ok(L.reff_info(h, p(inf)))
        fx[f"{tag}_info"] = inf
        fx[f"{tag}_sizes"], fx[f"{tag}_sha"] = lists_digest(h, pf.REF_NLIST, int(inf[5]))
        fx[f"{tag}_xq"] = xq
        for nprobe in (5, 8, 16):
            Dq, Iq = qsearch(h, xq, nprobe)
            fx[f"{tag}_q{nprobe}_D"], fx[f"{tag}_q{nprobe}_I"] = Dq, Iq
        for t in (1, 0):
            ok(L.reff_ivfpq_set_table(h, 1 if t == 1 else -1))
            for nprobe, k in pf.REF_CASES:
                D, I = preassigned(h, xq, k, fx[f"{tag}_q{nprobe}_I"], fx[f"{tag}_q{nprobe}_D"])
                fx[f"{tag}_t{t}_pre_{nprobe}_{k}_D"] = D
                fx[f"{tag}_t{t}_pre_{nprobe}_{k}_I"] = I
        ok(L.reff_ivfpq_set_table(h, 1))
        pr = pf.REF_PARAMS
        D = np.empty((pf.REF_NQ, pr["k"]), np.float32)
        I = np.empty((pf.REF_NQ, pr["k"]), np.int64)
        ok(L.reff_search_params(h, pf.REF_NQ, p(xq), pr["k"], pr["nprobe"], pr["max_codes"],
                                p(c["sel"]), c["sel"].size, p(D), p(I)))
        fx[f"{tag}_params_D"], fx[f"{tag}_params_I"], fx[f"{tag}_params_sel"] = D, I, c["sel"]
        L.reff_free(h)
    np.savez_compressed(OUT, **fx)
    tot = os.path.getsize(OUT)
    print(f"{OUT}: {tot} bytes, {len(fx)} arrays")
    for tag in pf.REF_TAGS:
        f = os.path.join(OUTD, tag + ".faiss")
        print(f"{f}: {os.path.getsize(f)} bytes")
        tot += os.path.getsize(f)
    print(f"total {tot} bytes")


if __name__ == "__main__":
    main()
