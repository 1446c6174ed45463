#!/usr/bin/env python3
"""Reference-run fixtures for IndexIVFPQ with 4- to 7-bit codes.

Writes tests/golden/ref_pq_nbits/<tag>.faiss and tests/golden/ref_pq_nbits.npz.
Runs only where oracle/_ref/libfaissfull.so exists (the reference CPU library
that `make -C oracle/ref full` compiles), through the reff_* entry points it
already exports: reff_index_factory, reff_train, reff_add, reff_write_index,
reff_quantizer_search, reff_search_preassigned, reff_search_params,
reff_range_search / _total / _copy, reff_assign, reff_encode_vectors,
reff_list_size / _copy, reff_ivfpq_set_table, reff_set_threads(1).

Recipe: nlist 16, 3000 training rows, 2000 added rows = 250 base rows repeated
8 times (row i is base row i mod 250) under shuffled ids, so the 8 copies of a
row share a list and a code, tie bit for bit, and arrive in an order that is not
their id order.  nq = 32 (>= 20: the flat quantizer's BLAS form), nprobe 4, one
OpenMP thread.  Inputs are ref_float_rand streams: the tests regenerate the
rows from the seeds in <tag>_meta.

reff_ivfpq_set_table(h, 0) lets the reference's precompute_table() choose again
(it chooses table 1 at these sizes); -1 disables the table, which is table 0.

The generator asserts, from the reference's own output, that at k = 10 every
query of every case has a tied group cut by the boundary.

    python scripts/make_golden_pq_nbits.py
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTD = os.path.join(ROOT, "tests", "golden", "ref_pq_nbits")
OUT = os.path.join(ROOT, "tests", "golden", "ref_pq_nbits.npz")

L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissfull.so"), mode=C.RTLD_GLOBAL)
P, I64 = C.c_void_p, C.c_int64
L.reff_last_error.restype = C.c_char_p
L.reff_index_factory.restype = P
L.reff_index_factory.argtypes = [C.c_int, C.c_char_p, C.c_int]
L.reff_write_index.argtypes = [P, C.c_char_p]
L.reff_free.argtypes = [P]
L.reff_train.argtypes = [P, I64, P]
L.reff_add.argtypes = [P, I64, P, P]
L.reff_set_threads.argtypes = [C.c_int]
L.reff_ivfpq_set_table.argtypes = [P, C.c_int]
L.reff_quantizer_search.argtypes = [P, I64, P, I64, P, P]
L.reff_search_preassigned.argtypes = [P, I64, P, I64, I64, P, P, C.c_int, P, P]
L.reff_search_params.argtypes = [P, I64, P, I64, I64, I64, P, I64, P, P]
L.reff_range_search.restype = P
L.reff_range_search.argtypes = [P, I64, P, C.c_float, I64]
L.reff_range_total.restype = I64
L.reff_range_total.argtypes = [P]
L.reff_range_copy.argtypes = [P, P, P, P]
L.reff_assign.argtypes = [P, I64, P, P]
L.reff_encode_vectors.argtypes = [P, I64, P, P, P]
L.reff_list_size.restype = I64
L.reff_list_size.argtypes = [P, I64]
L.reff_list_copy.argtypes = [P, I64, P, P]

REFP = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissref.so"))
REFP.ref_float_rand.argtypes = [P, C.c_size_t, C.c_int64]

NLIST, NT, NBASE, REP, NQ, NPROBE = 16, 3000, 250, 8, 32, 4
NB = NBASE * REP
MAX_CODES, NENC = 150, 64

# tag, factory, metric_l2, d, M, nbits, tables, ks, extras
CASES = [
    ("PQ16x4", "IVF16,PQ16x4", 1, 64, 16, 4, (1, -1), (1, 10, 100), ("range", "params", "encode")),
    ("PQ10x5", "IVF16,PQ10x5", 1, 40, 10, 5, (1, -1), (10,), ()),
    ("PQ32x6", "IVF16,PQ32x6", 1, 64, 32, 6, (-1,), (10,), ()),
    ("PQ24x7", "IVF16,PQ24x7", 1, 96, 24, 7, (-1,), (10,), ()),
    ("PQ16x4_ip", "IVF16,PQ16x4", 0, 64, 16, 4, (0,), (10,), ("range",)),
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


def data(d, seed):
    """(xt, xb, ids, xq): see the module docstring; the tests rebuild these."""
    xt = float_rand(NT, d, seed)
    xb = np.ascontiguousarray(np.tile(float_rand(NBASE, d, seed + 1), (REP, 1)))
    xq = float_rand(NQ, d, seed + 2)
    ids = np.random.RandomState(seed + 3).permutation(NB).astype(np.int64)
    return xt, xb, ids, xq


def boundary_ties(D, k):
    """Queries whose k-th distance equals the (k-1)-th or is shared by a row the
    result left out cannot be told from D alone; the copies make groups of 8,
    so: the value at the boundary occurs fewer than 8 times in the row."""
    n = 0
    for row in D:
        n += int(0 < (row == row[k - 1]).sum() < REP)
    return n


def main():
    os.makedirs(OUTD, exist_ok=True)
    L.reff_set_threads(1)
    fx = {}
    for ci, (tag, desc, ml2, d, M, nbits, tables, ks, extras) in enumerate(CASES):
        seed = 8100 + 10 * ci
        xt, xb, ids, xq = data(d, seed)
        h = L.reff_index_factory(d, desc.encode(), ml2)
        if not h:
            raise RuntimeError(L.reff_last_error().decode())
        ok(L.reff_train(h, NT, p(xt)))
        # the add path first, on the trained and still empty index
        if "encode" in extras:
            lst = np.empty(NENC, np.int64)
            ok(L.reff_assign(h, NENC, p(xb), p(lst)))
            codes = np.zeros((NENC, (M * nbits + 7) // 8), np.uint8)
            ok(L.reff_encode_vectors(h, NENC, p(xb), p(lst), p(codes)))
            fx[f"{tag}_enc_list"], fx[f"{tag}_enc_codes"] = lst.astype(np.int32), codes
        ok(L.reff_add(h, NB, p(xb), p(ids)))
        ok(L.reff_write_index(h, os.path.join(OUTD, tag + ".faiss").encode()))
        cs = (M * nbits + 7) // 8
        sizes = np.array([L.reff_list_size(h, l) for l in range(NLIST)], np.int64)
        lcodes = np.zeros((NB, cs), np.uint8)
        lids = np.zeros(NB, np.int64)
        o = 0
        for l in range(NLIST):
            if sizes[l]:
                ok(L.reff_list_copy(h, l, p(lcodes[o:o + sizes[l]]), p(lids[o:o + sizes[l]])))
            o += sizes[l]
        assert o == NB
        fx[f"{tag}_list_sizes"], fx[f"{tag}_list_codes"] = sizes.astype(np.int32), lcodes
        fx[f"{tag}_list_ids"] = lids.astype(np.int32)
        Dq = np.empty((NQ, NPROBE), np.float32)
        Iq = np.empty((NQ, NPROBE), np.int64)
        ok(L.reff_quantizer_search(h, NQ, p(xq), NPROBE, p(Dq), p(Iq)))
        # [d, nlist, nb, metric_l2, nprobe, nq, seed, M, nbits, nbase, nt]
        fx[f"{tag}_meta"] = np.array([d, NLIST, NB, ml2, NPROBE, NQ, seed, M, nbits, NBASE, NT],
                                     np.int64)
        fx[f"{tag}_tables"] = np.array(tables, np.int64)
        fx[f"{tag}_ks"] = np.array(ks, np.int64)
        fx[f"{tag}_Dq"], fx[f"{tag}_Iq"] = Dq, Iq.astype(np.int32)
        for t in tables:
            if ml2:
                ok(L.reff_ivfpq_set_table(h, t))
            tt = f"{tag}_t{max(t, 0)}"
            for k in ks:
                D = np.empty((NQ, k), np.float32)
                I = np.empty((NQ, k), np.int64)
                ok(L.reff_search_preassigned(h, NQ, p(xq), k, NPROBE, p(Iq), p(Dq), 0, p(D),
                                             p(I)))
                D2 = np.empty((NQ, k), np.float32)
                I2 = np.empty((NQ, k), np.int64)
                ok(L.reff_search_params(h, NQ, p(xq), k, NPROBE, 0, None, 0, p(D2), p(I2)))
                assert np.array_equal(D, D2) and np.array_equal(I, I2), "search != preassigned"
                fx[f"{tt}_{k}_D"], fx[f"{tt}_{k}_I"] = D, I.astype(np.int32)
                if k == 10:
                    cut = boundary_ties(D, k)
                    print(f"{tt}: {cut}/{NQ} queries have a tied group cut at k = 10")
                    assert cut == NQ, (tt, cut)
            if "range" in extras:
                radius = np.float32(np.median(fx[f"{tt}_10_D"][:, 5]))
                r = L.reff_range_search(h, NQ, p(xq), radius, NPROBE)
                if not r:
                    raise RuntimeError(L.reff_last_error().decode())
                tot = L.reff_range_total(r)
                lims = np.empty(NQ + 1, np.int64)
                RD = np.empty(max(tot, 1), np.float32)
                RI = np.empty(max(tot, 1), np.int64)
                L.reff_range_copy(r, p(lims), p(RD), p(RI))
                assert 0 < tot and (np.diff(lims) > 0).sum() >= NQ // 4
                fx[f"{tt}_radius"] = radius
                fx[f"{tt}_range_lims"] = lims
                fx[f"{tt}_range_D"], fx[f"{tt}_range_I"] = RD[:tot], RI[:tot].astype(np.int32)
                print(f"{tt}: range radius {radius}: {tot} hits")
            if "params" in extras:
                sel = np.ascontiguousarray(np.arange(0, NB, 3, dtype=np.int64))
                D = np.empty((NQ, 10), np.float32)
                I = np.empty((NQ, 10), np.int64)
                ok(L.reff_search_params(h, NQ, p(xq), 10, NPROBE, MAX_CODES, p(sel), len(sel),
                                        p(D), p(I)))
                assert (I >= 0).all() and (I % 3 == 0).all()
                fx[f"{tt}_params_D"], fx[f"{tt}_params_I"] = D, I.astype(np.int32)
        L.reff_free(h)
    np.savez_compressed(OUT, **fx)
    tot = os.path.getsize(OUT)
    print(f"{OUT}: {tot} bytes")
    assert tot < (1 << 20)
    for tag, *_ in CASES:
        f = os.path.join(OUTD, tag + ".faiss")
        sz = os.path.getsize(f)
        assert sz < (1 << 20), (f, sz)
        print(f"{f}: {sz} bytes")
        tot += sz
    print(f"total {tot} bytes")


if __name__ == "__main__":
    main()
