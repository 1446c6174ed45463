#!/usr/bin/env python3
"""Reference-run fixtures for IndexRefineFlat ("<base>,RFlat").

Writes tests/golden/ref_refine/<tag>.faiss and tests/golden/ref_refine.npz.
Runs only where oracle/_ref/libfaissfull.so exists (the reference CPU library
that `make -C oracle/ref full` compiles), through the reff_* entry points it
already exports: reff_index_factory, reff_train, reff_add (ids = NULL, so labels
are rows of the flat storage), reff_write_index, reff_read_index, reff_search,
reff_set_threads(1).

The wrapper hides the base index from reff_set_nprobe, and IndexRefine rejects
the SearchParametersIVF that reff_search_params passes, so nprobe and k_factor
are set *in the file*: the reference writes the index, this script patches the
two fields in the bytes (the base IVF index's nprobe, the second size_t after
its header, and k_factor, the file's last 4 bytes; nothing else changes and
this library's writer is not involved), and the reference reads the patched
file and searches it.  The patched file is the one committed.

Inputs are ref_float_rand streams, nq = 32 (>= 20: the flat coarse quantizer's
BLAS form), one OpenMP thread.

Planted ties.  In a sorted base row equal base distances already come in id
order, so duplicated rows cannot tell the reference's arrival-order tie rule
(reorder_2_heaps, faiss/IndexRefine.cpp:65-87) from a (distance, id) sort.
  * pq_l2_d64: queries 0..7 are rounded to multiples of 2^-6; for query j two
    base rows are overwritten with q_j + e_j and q_j - e_j, e_j a sparse vector
    of multiples of 2^-6.  Differences, squares and partial sums are exact in
    fp32, so the two rows tie bit for bit in exact distance, while their PQ
    codes — and so their ranks in the base result — differ.  The "+" row gets
    the smaller id for even j, the larger for odd j.
  * flat_ip_d40 / flat_ip_d44: queries 0..7 are rounded to multiples of 2^-4;
    the two rows are 2 q_j plus 1/2 on one of two dimensions where q_j has equal
    values (permutations of each other over those dimensions); every product
    and partial sum is exact, so their inner products tie bit for bit.  Their
    base index is IVF-Flat, whose distances are the exact ones: the pair ties
    in the base row too and arrives larger id first (the CMin heap's order), so
    these two cases pin the inner-product direction of the rule but a (distance
    descending, id descending) sort would pass them as well.
  * sq8_ip_d40: the same planted rows behind an IVF-SQ8 base, whose decoded
    distances differ per dimension, so the pair's base order is not its id
    order: this is the inner-product case that separates the two rules.
The generator asserts, from the reference's own results, that at k = 1 every
planted query returns a row of its pair and at least two per case return the
LARGER id — and, where the base distances are approximate (pq_l2_d64,
sq8_ip_d40), at least two the smaller; a case tries further seeds until that
holds and records the one used (meta[6]).

    python scripts/make_golden_refine.py
"""
import ctypes as C
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTD = os.path.join(ROOT, "tests", "golden", "ref_refine")
OUT = os.path.join(ROOT, "tests", "golden", "ref_refine.npz")

L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissfull.so"), mode=C.RTLD_GLOBAL)
P, I64 = C.c_void_p, C.c_int64
L.reff_last_error.restype = C.c_char_p
L.reff_index_factory.restype = P
L.reff_index_factory.argtypes = [C.c_int, C.c_char_p, C.c_int]
L.reff_read_index.restype = P
L.reff_read_index.argtypes = [C.c_char_p, C.c_int]
L.reff_write_index.argtypes = [P, C.c_char_p]
L.reff_free.argtypes = [P]
L.reff_train.argtypes = [P, I64, P]
L.reff_add.argtypes = [P, I64, P, P]
L.reff_search.argtypes = [P, I64, P, I64, P, P]
L.reff_set_threads.argtypes = [C.c_int]

REFP = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissref.so"))
REFP.ref_float_rand.argtypes = [P, C.c_size_t, C.c_int64]

NQ = 32
NPLANT = 8
HEADER = 33  # d:i32 ntotal:i64 dummy:i64 dummy:i64 is_trained:u8 metric:i32

# index name, factory, metric_l2, d, nlist, nb
INDEXES = [
    ("pq_l2_d64", "IVF32,PQ8,RFlat", 1, 64, 32, 2000),
    ("flat_ip_d40", "IVF16,Flat,RFlat", 0, 40, 16, 1500),
    ("flat_ip_d44", "IVF16,Flat,RFlat", 0, 44, 16, 1500),
    ("sq8_l2_d72", "IVF16,SQ8,RFlat", 1, 72, 16, 1200),
    ("pq_l2_d96_k1", "IVF16,PQ12,RFlat", 1, 96, 16, 1200),
    ("sq8_ip_d40", "IVF16,SQ8,RFlat", 0, 40, 16, 1500),
]
# tag, index name, nprobe, k_factor, ks
CASES = [
    ("pq_l2_d64", "pq_l2_d64", 4, 4.0, (1, 10, 64, 100)),
    ("pq_l2_d64_kf25", "pq_l2_d64", 4, 2.5, (3, 10)),
    ("pq_l2_d64_np1", "pq_l2_d64", 1, 4.0, (100,)),
    ("flat_ip_d40", "flat_ip_d40", 4, 3.0, (1, 10)),
    ("flat_ip_d44", "flat_ip_d44", 4, 3.0, (1, 10)),
    ("sq8_l2_d72", "sq8_l2_d72", 4, 4.0, (10,)),
    ("pq_l2_d96_k1", "pq_l2_d96_k1", 16, 1.0, (10,)),
    ("sq8_ip_d40", "sq8_ip_d40", 4, 3.0, (1, 10)),
]
PLANTED = ("pq_l2_d64", "flat_ip_d40", "flat_ip_d44", "sq8_ip_d40")
# base distances that differ from the exact ones: the planted pair's order in
# the base row is not its id order, so both ids must win somewhere
APPROX_BASE = ("pq_l2_d64", "sq8_ip_d40")


def p(a):
    return a.ctypes.data_as(P) if a is not None else None


def ok(rc):
    if rc != 0:
        raise RuntimeError(L.reff_last_error().decode())


def float_rand(n, d, seed):
    x = np.empty(n * d, np.float32)
    REFP.ref_float_rand(p(x), n * d, seed)
    return x.reshape(n, d)


def plant(name, ml2, xb, xq, seed):
    """Overwrite queries 0..NPLANT-1 and two base rows each; returns
    [NPLANT][3] = (query, id of the "+" row, id of the "-" row)."""
    rng = np.random.RandomState(seed)
    nb, d = xb.shape
    rows = rng.choice(nb, 2 * NPLANT, replace=False)
    pairs = np.zeros((NPLANT, 3), np.int64)
    for j in range(NPLANT):
        lo, hi = sorted(int(r) for r in rows[2 * j:2 * j + 2])
        plus, minus = (lo, hi) if j % 2 == 0 else (hi, lo)
        if ml2:
            q = np.round(xq[j] * 64) / 64
            e = np.zeros(d, np.float32)
            dims = rng.choice(d, 24, replace=False)
            e[dims] = rng.choice([-1, 1], 24) * rng.randint(4, 17, 24) / 64.0
            xq[j] = q
            xb[plus], xb[minus] = q + e, q - e
            assert float((e * e).sum()) < 1.5
        else:
            q = np.round(xq[j] * 16) / 16
            order = np.argsort(q, kind="stable")
            same = [(a, b) for a, b in zip(order[:-1], order[1:]) if q[a] == q[b] and q[a] > 0]
            i1, i2 = same[rng.randint(len(same))]
            xq[j] = q
            xb[plus], xb[minus] = 2 * q, 2 * q
            xb[plus, i1] += 0.5
            xb[minus, i2] += 0.5
        pairs[j] = (j, plus, minus)
    return pairs


def patch(path, nprobe, k_factor):
    """nprobe of the base IVF index and k_factor, in the file's bytes."""
    b = bytearray(open(path, "rb").read())
    assert b[:4] == b"IxRF" and bytes(b[4 + HEADER:8 + HEADER]) in (b"IwPQ", b"IwFl", b"IwSq")
    off = 4 + HEADER + 4 + HEADER + 8  # IxRF, header, IwXX, header, nlist
    assert struct.unpack_from("<Q", b, off)[0] == 1  # the factory's nprobe
    assert struct.unpack_from("<f", b, len(b) - 4)[0] == 1.0  # ... and k_factor
    struct.pack_into("<Q", b, off, nprobe)
    struct.pack_into("<f", b, len(b) - 4, k_factor)
    return bytes(b)


def search(h, xq, k):
    D = np.empty((xq.shape[0], k), np.float32)
    I = np.empty((xq.shape[0], k), np.int64)
    ok(L.reff_search(h, xq.shape[0], p(xq), k, p(D), p(I)))
    return D, I


def build(name, desc, ml2, d, nlist, nb, seed):
    """The reference builds and writes the index; returns (raw path, xq, pairs)."""
    h = L.reff_index_factory(d, desc.encode(), ml2)
    if not h:
        raise RuntimeError(L.reff_last_error().decode())
    xb = float_rand(nb, d, seed)
    xq = float_rand(NQ, d, seed + 1)
    pairs = np.zeros((0, 3), np.int64)
    if name in PLANTED:
        pairs = plant(name, ml2, xb, xq, seed + 2)
    ok(L.reff_train(h, nb, p(xb)))
    ok(L.reff_add(h, nb, p(xb), None))
    raw = os.path.join(OUTD, name + ".raw")
    ok(L.reff_write_index(h, raw.encode()))
    L.reff_free(h)
    return raw, xq, pairs


def run_case(tag, raw, nprobe, k_factor, ks, xq):
    path = os.path.join(OUTD, tag + ".faiss")
    with open(path, "wb") as f:
        f.write(patch(raw, nprobe, k_factor))
    h = L.reff_read_index(path.encode(), 0)
    if not h:
        raise RuntimeError(L.reff_last_error().decode())
    out = {k: search(h, xq, k) for k in ks}
    L.reff_free(h)
    return out


def larger_id_wins(pairs, I1):
    """Queries whose k = 1 result is the larger id of their pair; -1 when some
    planted query does not return a row of its pair."""
    n = 0
    for j, plus, minus in pairs:
        if I1[j, 0] not in (plus, minus):
            return -1
        n += int(I1[j, 0] == max(plus, minus))
    return n


def main():
    os.makedirs(OUTD, exist_ok=True)
    fx = {}
    L.reff_set_threads(1)
    built = {}
    for ci, (name, desc, ml2, d, nlist, nb) in enumerate(INDEXES):
        first = next(c for c in CASES if c[1] == name)
        for attempt in range(32):
            seed = 7300 + 100 * ci + 3 * attempt
            raw, xq, pairs = build(name, desc, ml2, d, nlist, nb, seed)
            if len(pairs) == 0:
                break
            res = run_case(first[0], raw, first[2], first[3], (1,), xq)
            wins = larger_id_wins(pairs, res[1][1])
            print(f"{name}: seed {seed}: {wins}/{NPLANT} planted queries return the larger id")
            if 2 <= wins <= NPLANT - (2 if name in APPROX_BASE else 0):
                break
        else:
            raise RuntimeError(f"{name}: no seed separates arrival order from id order")
        built[name] = (raw, xq, pairs, seed, ml2, d, nlist, nb)
    for tag, name, nprobe, k_factor, ks in CASES:
        raw, xq, pairs, seed, ml2, d, nlist, nb = built[name]
        out = run_case(tag, raw, nprobe, k_factor, ks, xq)
        # [d, nlist, nb, metric_l2, nprobe, nq, seed]
        fx[f"{tag}_meta"] = np.array([d, nlist, nb, ml2, nprobe, NQ, seed], np.int64)
        fx[f"{tag}_k_factor"] = np.float32(k_factor)
        fx[f"{tag}_ks"] = np.array(ks, np.int64)
        fx[f"{tag}_xq"] = xq
        fx[f"{tag}_pairs"] = pairs
        for k, (D, I) in out.items():
            fx[f"{tag}_{k}_D"], fx[f"{tag}_{k}_I"] = D, I.astype(np.int32)
    for name in built:
        os.remove(built[name][0])
    # the padded case really pads, and the k_base = 7 case really truncates
    assert (fx["pq_l2_d64_np1_100_I"] < 0).any()
    np.savez_compressed(OUT, **fx)
    tot = os.path.getsize(OUT)
    print(f"{OUT}: {tot} bytes")
    for tag, *_ in CASES:
        f = os.path.join(OUTD, tag + ".faiss")
        sz = os.path.getsize(f)
        assert sz < (1 << 20), (f, sz)
        print(f"{f}: {sz} bytes")
        tot += sz
    print(f"total {tot} bytes")


if __name__ == "__main__":
    main()
