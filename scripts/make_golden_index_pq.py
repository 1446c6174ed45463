#!/usr/bin/env python3
"""Reference-run fixtures for IndexPQ (file tag IxPq).

Writes tests/golden/ref_index_pq/<tag>.faiss and <tag>.npz.  Runs only where
oracle/_ref/libfaissfull.so exists (the reference CPU library that
`make -C oracle/ref full` compiles).  No training: codebooks and codes are
random, the IxPq file is laid out here in numpy (faiss/impl/index_write.cpp:
417-425), read by the reference (oracle/reflib.py), written back by it (the
committed file is the reference's own bytes; they must equal numpy's) and
searched on one thread.  Recorded: the queries and the reference's D, I for
k = 10.

Planted ties: for every query the rows ranked 1st, 9th and 10th (float64)
are copied over two other rows each, so equal distances sit inside the result
and straddle the k boundary.

    python scripts/make_golden_index_pq.py
"""
import ctypes as C
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTD = os.path.join(ROOT, "tests", "golden", "ref_index_pq")
sys.path.insert(0, ROOT)
from oracle import reflib  # noqa: E402

NB, NQ, K = 300, 8, 10
# tag, d, M, nbits, metric (1 = L2, 0 = inner product)
CASES = [("pq8x8_l2", 32, 8, 8, 1), ("pq8x8_ip", 32, 8, 8, 0), ("pq16x8_l2", 64, 16, 8, 1),
         ("pq5x5_l2", 20, 5, 5, 1), ("pq12x6_ip", 48, 12, 6, 0), ("pq16x4_l2", 32, 16, 4, 1),
         ("pq2x8_dsub16_l2", 32, 2, 8, 1)]


def pack(idx, nbits):
    """PQEncoderGeneric: index m in bits [m nbits, (m + 1) nbits), little endian."""
    n, M = idx.shape
    out = np.zeros((n, (M * nbits + 7) // 8), np.uint8)
    for m in range(M):
        o = m * nbits
        v = idx[:, m].astype(np.uint32) << (o & 7)
        out[:, o >> 3] |= (v & 255).astype(np.uint8)
        if (o & 7) + nbits > 8:
            out[:, (o >> 3) + 1] |= (v >> 8).astype(np.uint8)
    return out


def ixpq_bytes(d, M, nbits, metric, cent, codes):
    n = codes.shape[0]
    b = b"IxPq" + struct.pack("<iqqqBi", d, n, 1 << 20, 1 << 20, 1, metric)
    b += struct.pack("<QQQQ", d, M, nbits, cent.size) + cent.astype("<f4").tobytes()
    b += struct.pack("<Q", codes.size) + codes.tobytes()
    return b + struct.pack("<iBi", 0, 0, 0)  # ST_PQ, encode_signs, polysemous_ht


def main():
    os.makedirs(OUTD, exist_ok=True)
    L = reflib.lib()
    L.reff_write_index.argtypes = [C.c_void_p, C.c_char_p]
    for ci, (tag, d, M, nbits, metric) in enumerate(CASES):
        rng = np.random.default_rng(4100 + ci)
        dsub, ksub = d // M, 1 << nbits
        cent = rng.standard_normal((M, ksub, dsub)).astype(np.float32)
        idx = rng.integers(0, ksub, (NB, M))
        xq = rng.standard_normal((NQ, d)).astype(np.float32)
        dec = cent[np.arange(M), idx].reshape(NB, d).astype(np.float64)
        ref = (((xq[:, None, :].astype(np.float64) - dec[None]) ** 2).sum(-1) if metric
               else -(xq.astype(np.float64) @ dec.T))
        spare = iter(rng.permutation(NB))
        order = np.argsort(ref, axis=1, kind="stable")
        for q in range(NQ):
            for r in (0, K - 2, K - 1):
                for _ in range(2):
                    idx[next(spare)] = idx[order[q, r]]
        codes = pack(idx, nbits)
        blob = ixpq_bytes(d, M, nbits, metric, cent, codes)
        path = os.path.join(OUTD, tag + ".faiss")
        with open(path + ".np", "wb") as f:
            f.write(blob)
        ix = reflib.RefIndex(path + ".np")
        assert L.reff_write_index(ix.h, path.encode()) == 0, L.reff_last_error().decode()
        os.remove(path + ".np")
        assert open(path, "rb").read() == blob, f"{tag}: the reference writes other bytes"
        Dr, Ir = ix.search(xq, K, 1)
        ties = int((Dr[:, 1:] == Dr[:, :-1]).sum())
        np.savez(os.path.join(OUTD, tag + ".npz"), xq=xq, D=Dr, I=Ir)
        print(f"{tag}: {len(blob)} bytes, {ties} equal neighbours in D")


if __name__ == "__main__":
    main()
