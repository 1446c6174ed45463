#!/usr/bin/env python3
"""Reference-run fixtures on the distributions of tests/hard_data.py: signed,
offset (cancellation), one dominant coordinate, near-ties, zero rows and
non-finite rows.  Same driver library and protocol as make_golden_full.py (one
OpenMP thread at search, nq = 64 so the flat coarse quantizer takes its BLAS
form); every expected array is an output of the reference's own code.

Writes
  tests/golden/ref_hard/<tag>.faiss  the reference-written index
  tests/golden/ref_hard/<tag>.npz    the reference's results over that index
  tests/golden/ref_hard.npz          the inputs: the queries of every
                                     distribution and the sha256 of every
                                     database (the rows themselves are in the
                                     flat index files)
The archives are written with fixed zip timestamps, so a second run gives the
same bytes.

`nonfinite`: the reference's k-means is not run on non-finite rows and its
coarse quantizer assigns them to no list (label -1), so the index is trained on
the clean copy (hard_data.clean), the list numbers are the clean copy's
(quantizer->assign) and the altered rows are added with IndexIVF::add_core
under those numbers.  The altered rows lie in several lists and 64-row tiles,
row 0 first in its list (asserted below).

    python oracle/ref/make_golden_hard.py
"""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hard_data  # noqa: E402
import make_golden_full as G  # noqa: E402  (the driver's ctypes prototypes and helpers)

L, p, ok = G.L, G.p, G.ok
L.reff_add_core.argtypes = [G.P, G.I64, G.P, G.P, G.P]

OUTD = os.path.join(ROOT, "tests", "golden", "ref_hard")
OUT = os.path.join(ROOT, "tests", "golden", "ref_hard.npz")
NB, NQ, NLIST, SEED = 2048, 64, 8, 9000

L2_DISTS = ["signed", "offset1", "offset4", "offset100", "heavy", "tight", "sparse", "nonfinite"]
IP_DISTS = ["signed", "sparse", "heavy", "nonfinite"]
PQ_DISTS = ["signed", "offset4", "heavy"]
SQ_DISTS = ["signed", "offset4"]
HNSW_DISTS = ["signed", "offset100", "tight"]


def savez(path, arrays):
    """np.savez_compressed with fixed member timestamps (reproducible bytes)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def data(dist, d):
    xb = hard_data.make(dist, NB, d, SEED + d)
    return xb, hard_data.queries(dist, xb, NQ, SEED + d)


def build_ivf(desc, d, ml2, dist):
    xb, xq = data(dist, d)
    h = L.reff_index_factory(d, desc.encode(), ml2)
    if not h:
        raise RuntimeError(L.reff_last_error().decode())
    L.reff_set_threads(8)
    xt = hard_data.clean(dist, xb)
    ok(L.reff_train(h, NB, p(xt)))
    if dist == "nonfinite":
        la = np.empty(NB, np.int64)
        ok(L.reff_assign(h, NB, p(xt), p(la)))
        ok(L.reff_add_core(h, NB, p(xb), None, p(la)))
        rows = [r for r, _, _ in hard_data.NONFINITE_ROWS]
        pos = [int((la[:r] == la[r]).sum()) for r in rows]
        assert pos[0] == 0, pos
        assert len({int(la[r]) for r in rows}) >= 2, la[rows]
        assert len({q // 64 for q in pos}) >= 3, pos
    else:
        ok(L.reff_add(h, NB, p(xb), None))
    L.reff_set_threads(1)
    return h, xb, xq


def record_ivf(h, xq, tables=(None,)):
    fx = {"info": G.info(h)}
    for nprobe in (4, 8):
        Dq, Iq = G.qsearch(h, xq, nprobe)
        fx[f"q{nprobe}_D"], fx[f"q{nprobe}_I"] = Dq, Iq
        for t in tables:
            if t is not None:
                ok(L.reff_ivfpq_set_table(h, 1 if t == 1 else -1))
            pre = "" if t is None else f"t{t}_"
            for k in (1, 10, 100):
                D, I = G.preassigned(h, xq, k, Iq, Dq)
                fx[f"{pre}pre_{nprobe}_{k}_D"], fx[f"{pre}pre_{nprobe}_{k}_I"] = D, I
    if tables != (None,):
        ok(L.reff_ivfpq_set_table(h, 1))
    for nprobe, k in ((4, 10), (8, 1)):
        ok(L.reff_set_nprobe(h, nprobe))
        D, I = G.search(h, xq, k)
        fx[f"full_{nprobe}_{k}_D"], fx[f"full_{nprobe}_{k}_I"] = D, I
    return fx


def finish(h, tag, fx):
    ok(L.reff_write_index(h, os.path.join(OUTD, tag + ".faiss").encode()))
    savez(os.path.join(OUTD, tag + ".npz"), fx)
    L.reff_free(h)


def main():
    os.makedirs(OUTD, exist_ok=True)
    inputs = {}

    def note(dist, d, xb, xq):
        inputs[f"{dist}_d{d}_xq"] = xq
        inputs[f"{dist}_d{d}_xb_sha"] = np.frombuffer(hashlib.sha256(xb.tobytes()).digest(),
                                                      np.uint8)

    for ml2, dists in ((1, L2_DISTS), (0, IP_DISTS)):
        for dist in dists:
            h, xb, xq = build_ivf(f"IVF{NLIST},Flat", 64, ml2, dist)
            note(dist, 64, xb, xq)
            finish(h, f"flat_{'l2' if ml2 else 'ip'}_{dist}", record_ivf(h, xq))
    h, xb, xq = build_ivf(f"IVF{NLIST},Flat", 36, 1, "offset4")
    note("offset4", 36, xb, xq)
    finish(h, "flat_l2_d36_offset4", record_ivf(h, xq))

    for desc, fam in ((f"IVF{NLIST},PQ16", "pq8"), (f"IVF{NLIST},PQ16x4", "pq4")):
        for dist in PQ_DISTS:
            h, xb, xq = build_ivf(desc, 64, 1, dist)
            finish(h, f"{fam}_{dist}", record_ivf(h, xq, tables=(1, 0)))
    for desc, fam in ((f"IVF{NLIST},SQ8", "sq8"), (f"IVF{NLIST},SQfp16", "sqfp16")):
        for dist in SQ_DISTS:   # signed: a negative vmin
            h, xb, xq = build_ivf(desc, 64, 1, dist)
            finish(h, f"{fam}_{dist}", record_ivf(h, xq))

    for dist in HNSW_DISTS:
        xb, xq = data(dist, 64)
        h = L.reff_index_factory(64, b"HNSW16,Flat", 1)
        L.reff_set_threads(1)
        ok(L.reff_add(h, NB, p(xb), None))
        fx = {}
        for ef in (16, 64):
            ok(L.reff_set_hnsw_efsearch(h, ef))
            fx[f"ef{ef}_10_D"], fx[f"ef{ef}_10_I"] = G.search(h, xq, 10)
        finish(h, f"hnsw_{dist}", fx)

    savez(OUT, inputs)
    sizes = {f: os.path.getsize(os.path.join(OUTD, f)) for f in sorted(os.listdir(OUTD))}
    assert max(sizes.values()) < (1 << 20), sizes
    print(f"wrote {len(sizes)} files, {sum(sizes.values()) / 1e6:.2f} MB, largest "
          f"{max(sizes.values()) / 1e3:.0f} kB; {OUT} {os.path.getsize(OUT) / 1e3:.0f} kB")


if __name__ == "__main__":
    sys.exit(main())
