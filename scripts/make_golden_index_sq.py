#!/usr/bin/env python3
"""Reference-run fixtures for IndexScalarQuantizer (file tag IxSQ).

Writes tests/golden/ref_index_sq/<tag>.faiss and <tag>.npz.  Runs only where
oracle/_ref/libfaissfull.so exists (the reference CPU library that
`make -C oracle/ref full` compiles).  Trained ranges and codes are random, the
IxSQ file is laid out here in numpy (faiss/impl/index_write.cpp:234-241,
596-603), read by the reference (oracle/reflib.py), written back by it (the
committed file is the reference's own bytes; they must equal numpy's) and
searched on one thread.  Recorded: the queries and the reference's D, I for
k = 10.

Planted ties: for every query the rows ranked 1st, 9th and 10th (float64)
are copied over two other rows each, so equal distances sit inside the result
and straddle the k boundary.

One more case, train_add: the reference trains an empty, untrained SQ8 file on
300 float_rand rows and adds them; recorded are the rows and the trained
vector and codes of the file it then writes.

    python scripts/make_golden_index_sq.py
"""
import ctypes as C
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTD = os.path.join(ROOT, "tests", "golden", "ref_index_sq")
sys.path.insert(0, ROOT)
from oracle import oracle, reflib  # noqa: E402

NB, NQ, K = 300, 8, 10
QT_8bit, QT_fp16 = 0, 4
# tag, d, qtype, metric (1 = L2, 0 = inner product)
CASES = [("sq8_l2_d40", 40, QT_8bit, 1), ("sq8_ip_d72", 72, QT_8bit, 0),
         ("sqfp16_l2_d24", 24, QT_fp16, 1)]
TRAIN_D = 32


def ixsq_bytes(d, qtype, metric, trained, codes, is_trained=1):
    code_size = d * (2 if qtype == QT_fp16 else 1)
    n = codes.size // code_size
    b = b"IxSQ" + struct.pack("<iqqqBi", d, n, 1 << 20, 1 << 20, is_trained, metric)
    b += struct.pack("<iifQQ", qtype, 0, 0.0, d, code_size)  # RS_minmax, rangestat_arg 0
    b += struct.pack("<Q", trained.size) + trained.astype("<f4").tobytes()
    return b + struct.pack("<Q", codes.size) + codes.tobytes()


def parse_ixsq(blob, d):
    """(trained, codes) of an IxSQ file with an L2 / inner-product header."""
    o = 4 + struct.calcsize("<iqqqBi") + struct.calcsize("<iifQQ")
    (nt,) = struct.unpack_from("<Q", blob, o)
    trained = np.frombuffer(blob, "<f4", nt, o + 8)
    o += 8 + 4 * nt
    (nc,) = struct.unpack_from("<Q", blob, o)
    return trained.copy(), np.frombuffer(blob, np.uint8, nc, o + 8).reshape(-1, d).copy()


def main():
    os.makedirs(OUTD, exist_ok=True)
    L = reflib.lib()
    L.reff_write_index.argtypes = [C.c_void_p, C.c_char_p]
    L.reff_train.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.reff_add.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    for ci, (tag, d, qtype, metric) in enumerate(CASES):
        rng = np.random.default_rng(5200 + ci)
        xq = rng.standard_normal((NQ, d)).astype(np.float32)
        if qtype == QT_8bit:
            trained = np.concatenate([rng.standard_normal(d) - 1.0,
                                      rng.uniform(0.5, 3.0, d)]).astype(np.float32)
            rows = rng.integers(0, 256, (NB, d), dtype=np.uint8)
            dec = ((rows + 0.5) / 255.0 * trained[d:].astype(np.float64) + trained[:d])
        else:
            trained = np.zeros(0, np.float32)
            rows = rng.standard_normal((NB, d)).astype("<f2")
            dec = rows.astype(np.float64)
        ref = (((xq[:, None, :].astype(np.float64) - dec[None]) ** 2).sum(-1) if metric
               else -(xq.astype(np.float64) @ dec.T))
        spare = iter(rng.permutation(NB))
        order = np.argsort(ref, axis=1, kind="stable")
        for q in range(NQ):
            for r in (0, K - 2, K - 1):
                for _ in range(2):
                    rows[next(spare)] = rows[order[q, r]]
        codes = np.ascontiguousarray(rows).view(np.uint8)
        blob = ixsq_bytes(d, qtype, metric, trained, codes)
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

    d = TRAIN_D
    x = oracle.float_rand(NB * d, 7301).reshape(NB, d)
    tmp = os.path.join(OUTD, "train_add.tmp")
    with open(tmp, "wb") as f:
        f.write(ixsq_bytes(d, QT_8bit, 1, np.zeros(0, np.float32), np.zeros(0, np.uint8), 0))
    ix = reflib.RefIndex(tmp)
    L.reff_set_threads(1)
    assert L.reff_train(ix.h, NB, x.ctypes.data_as(C.c_void_p)) == 0, L.reff_last_error().decode()
    assert L.reff_add(ix.h, NB, x.ctypes.data_as(C.c_void_p), None) == 0, L.reff_last_error().decode()
    assert L.reff_write_index(ix.h, tmp.encode()) == 0, L.reff_last_error().decode()
    trained, codes = parse_ixsq(open(tmp, "rb").read(), d)
    os.remove(tmp)
    assert trained.size == 2 * d and codes.shape == (NB, d)
    np.savez(os.path.join(OUTD, "train_add.npz"), x=x, trained=trained, codes=codes)
    print(f"train_add: d = {d}, {NB} rows, codes span {codes.min()} .. {codes.max()}")


if __name__ == "__main__":
    main()
