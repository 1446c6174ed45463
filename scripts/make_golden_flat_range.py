#!/usr/bin/env python3
"""Reference-run fixtures for IndexFlat::range_search.

Writes tests/golden/ref_flat_range.npz (data only).  Runs only where
oracle/_ref/libfaissfull.so exists (the reference CPU library that
`make -C oracle/ref full` compiles), through the reff_* entry points it already
exports, one OpenMP thread: reff_index_factory(d, "Flat", metric), reff_add,
reff_search, reff_range_search (its nprobe argument is ignored by a flat
index; the SearchParametersIVF it passes carries no selector), reff_range_total,
reff_range_copy.

The databases are ref_float_rand streams with planted rows
(tests/flat_range_ref.py make_base); the file stores (rows, d, seed) and the
SHA-256 of the database bytes, the queries and the results in full, as a few
concatenated arrays (layout: tests/flat_range_ref.py case_arrays).

Cases, ntotal = 1337:
  * {l2, ip} x d in {13, 40, 128} x nq in {37, 19}: nq = 37 is the BLAS form
    (one full 32-row group plus a tail), nq = 19 the direct form (one below
    distance_compute_blas_threshold).  Radius: the median over the queries of
    the reference's k-NN distance at rank 12.
  * bnd_{l2, ip} (d = 40, nq = 37): the radius is the exact distance the
    reference's search returned for query 0 at rank 10, so the strict
    comparison excludes that row for query 0.
  * cancel_l2 (d = 40, nq = 37): database and queries shifted by +100, 8
    database rows equal to 8 of the queries; the radius is the smallest of
    query CLUSTER_QUERY's k-NN distances that leaves it more than 64 hits, a
    few fp32 ulps of |x|^2 + |y|^2, so the BLAS form's clamp and its
    cancellation noise decide the hits.
Asserted on every case, from the reference's own output: some query has no
hit, some query has more than 64 hits inside one 128-row tile, the total is
below 5% of the pairs, and hits come in ascending row order.

    python scripts/make_golden_flat_range.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flat_range_ref as fr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_flat_range.npz")

L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissfull.so"), mode=C.RTLD_GLOBAL)
P, I64 = C.c_void_p, C.c_int64
L.reff_last_error.restype = C.c_char_p
L.reff_index_factory.restype = P
L.reff_index_factory.argtypes = [C.c_int, C.c_char_p, C.c_int]
L.reff_free.argtypes = [P]
L.reff_add.argtypes = [P, I64, P, P]
L.reff_search.argtypes = [P, I64, P, I64, P, P]
L.reff_range_search.restype = P
L.reff_range_search.argtypes = [P, I64, P, C.c_float, I64]
L.reff_range_total.restype = I64
L.reff_range_total.argtypes = [P]
L.reff_range_copy.argtypes = [P, P, P, P]
L.reff_set_threads.argtypes = [C.c_int]

REFP = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissref.so"))
REFP.ref_float_rand.argtypes = [P, C.c_size_t, C.c_int64]

# group, kind, metric_l2, d, seed
GROUPS = [(f"{kind}_d{d}", kind, int(kind == "l2"), d, 8100 + 10 * i + (0 if kind == "l2" else 5))
          for kind in ("l2", "ip") for i, d in enumerate((13, 40, 128))]
GROUPS.append(("offset_d40", "offset", 1, 40, 8190))
# tag, group, nq, radius rule
CASES = [(f"{g}_nq{nq}", g, nq, "median") for g, kind, *_ in GROUPS if kind != "offset"
         for nq in (37, 19)]
CASES += [("bnd_l2", "l2_d40", 37, "boundary"), ("bnd_ip", "ip_d40", 37, "boundary"),
          ("cancel_l2", "offset_d40", 37, "cancel")]
KNN_RANK = 12    # "median": radius = median over queries of the 12th k-NN distance
BND_RANK = 10    # "boundary": radius = query 0's 10th k-NN distance


def p(a):
    return a.ctypes.data_as(P) if a is not None else None


def ok(rc):
    if rc != 0:
        raise RuntimeError(L.reff_last_error().decode())


def float_rand(n, seed):
    x = np.empty(n, np.float32)
    REFP.ref_float_rand(p(x), n, seed)
    return x


def search(h, xq, k):
    D = np.empty((xq.shape[0], k), np.float32)
    I = np.empty((xq.shape[0], k), np.int64)
    ok(L.reff_search(h, xq.shape[0], p(xq), k, p(D), p(I)))
    return D, I


def range_search(h, xq, radius):
    r = L.reff_range_search(h, xq.shape[0], p(xq), radius, 1)
    if not r:
        raise RuntimeError(L.reff_last_error().decode())
    tot = L.reff_range_total(r)
    lims = np.empty(xq.shape[0] + 1, np.int64)
    D = np.empty(max(tot, 1), np.float32)
    I = np.empty(max(tot, 1), np.int64)
    L.reff_range_copy(r, p(lims), p(D), p(I))
    return lims, D[:tot], I[:tot]


def main():
    L.reff_set_threads(1)
    fx = {}
    built = {}
    gnames = [g[0] for g in GROUPS]
    gmeta, gkind, gxq, gsha = [], [], [], []
    cgroup, cnq, cradius, clims, cD, cI = [], [], [], [], [], []
    for g, kind, ml2, d, seed in GROUPS:
        xq = fr.make_queries(float_rand, kind, d, seed + 1)
        xb = fr.make_base(float_rand, kind, d, seed, xq)
        h = L.reff_index_factory(d, b"Flat", ml2)
        if not h:
            raise RuntimeError(L.reff_last_error().decode())
        ok(L.reff_add(h, fr.NB, p(xb), None))
        built[g] = (h, xq, ml2)
        # [rows, d, seed, metric_l2]; kind; queries; SHA-256 of the database
        gmeta.append([fr.NB, d, seed, ml2])
        gkind.append(kind)
        gxq.append(xq.ravel())
        gsha.append(fr.sha256(xb))
    for tag, g, nq, rule in CASES:
        h, xq, ml2 = built[g]
        x = np.ascontiguousarray(xq[:nq])
        Dk, Ik = search(h, x, 128)
        if rule == "median":
            radius = np.float32(np.median(Dk[:, KNN_RANK - 1]))
        elif rule == "boundary":
            radius = Dk[0, BND_RANK - 1]
        else:
            # the smallest k-NN distance of the cluster's query that leaves
            # it more than 64 hits under the strict comparison
            row = Dk[fr.CLUSTER_QUERY]
            radius = next(v for v in np.unique(row) if (row < v).sum() > 64)
        radius = np.float32(radius)
        lims, D, I = range_search(h, x, float(radius))
        cnt = np.diff(lims)
        # the conditions every case meets, from the reference's own output
        assert (cnt == 0).any(), tag
        best = 0
        for i in range(nq):
            Ii = I[lims[i]:lims[i + 1]]
            assert np.all(np.diff(Ii) > 0), (tag, i)      # ascending rows
            if Ii.size:
                best = max(best, int(np.bincount(Ii // 128).max()))
        assert best > 64, (tag, best)
        assert lims[-1] < 0.05 * nq * fr.NB, (tag, int(lims[-1]))
        assert np.all(D < radius) if ml2 else np.all(D > radius), tag
        if rule == "boundary":
            I0 = I[lims[0]:lims[1]]
            assert Ik[0, BND_RANK - 1] not in I0, tag     # distance == radius: excluded
            assert set(Ik[0, :BND_RANK - 1]) <= set(I0.tolist()), tag
        if rule == "cancel":
            # pairs of equal vectors: whatever the reference returns for them
            for qi, rj in zip(fr.EQUAL_QUERIES, fr.EQUAL_ROWS):
                Ii = I[lims[qi]:lims[qi + 1]]
                print(f"  {tag}: query {qi} = row {rj}: "
                      f"{'hit ' + repr(float(D[lims[qi]:lims[qi + 1]][Ii == rj][0])) if rj in Ii else 'no hit'}")
        cgroup.append(gnames.index(g))
        cnq.append(nq)
        cradius.append(radius)
        clims.append(lims)
        cD.append(D)
        cI.append(I)
        print(f"{tag}: radius {float(radius)!r} total {int(lims[-1])} "
              f"({100.0 * lims[-1] / (nq * fr.NB):.2f}% of the pairs), max per tile {best}, "
              f"{int((cnt == 0).sum())} queries without a hit")
    for h, _, _ in built.values():
        L.reff_free(h)
    # the layout tests/flat_range_ref.py case_arrays / load_case read
    assert fr.NB <= 1 << 16
    fx["groups"] = np.array(gnames)
    fx["group_meta"] = np.array(gmeta, np.int32)
    fx["group_kind"] = np.array(gkind)
    fx["group_sha256"] = np.array(gsha)
    fx["xq"] = np.concatenate(gxq).astype(np.float32)
    fx["cases"] = np.array([c[0] for c in CASES])
    fx["case_group"] = np.array(cgroup, np.int32)
    fx["case_nq"] = np.array(cnq, np.int32)
    fx["case_radius"] = np.array(cradius, np.float32)
    fx["lims"] = np.concatenate(clims).astype(np.int32)
    fx["D"] = np.concatenate(cD).astype(np.float32)
    fx["I"] = np.concatenate(cI).astype(np.uint16)
    np.savez_compressed(OUT, **fx)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
