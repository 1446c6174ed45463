"""Shared by the IndexFlat range-search tests and the fixture generator
(scripts/make_golden_flat_range.py): how a fixture case's database is rebuilt
from its float_rand stream, and the host restatement of
IndexFlat::range_search (faiss/IndexFlat.cpp:71-90 ->
faiss/utils/distances.cpp:940-966 with a RangeSearchBlockResultHandler).

Database kinds (every one is ref_float_rand(rows * d, seed), then exact fp32
elementwise steps, then planted rows taken from the stored queries):
    "l2"      the stream as it is (uniform in [0, 1))
    "ip"      the stream minus 1/2 (signed: a random pair's inner product is
              near 0, a row's with itself near d / 12)
    "offset"  the stream plus 100 (tests/hard_data.py "offset100": |x|^2 + |y|^2
              dwarfs the distances, the BLAS form's result is cancellation
              noise and its clamp)
Planted rows: CLUSTER_ROWS (inside the one 128-row tile [256, 384)) are
scaled / shifted copies of query CLUSTER_QUERY, so that query has more than 64
hits inside one tile; "offset" also makes EQUAL_ROWS[i] = query EQUAL_QUERIES[i].
"""
import hashlib
import os

import numpy as np

NB = 1337
NQ_MAX = 37
CLUSTER_QUERY = 3
CLUSTER_ROWS = np.arange(260, 380)   # 120 rows of tile 2
NOHIT_QUERY = 5
EQUAL_ROWS = np.array([3, 130, 255, 256, 700, 1023, 1024, 1336])
EQUAL_QUERIES = np.array([0, 7, 11, 13, 19, 24, 30, 36])


def shift(kind):
    return {"l2": 0.0, "ip": -0.5, "offset": 100.0}[kind]


def make_queries(float_rand, kind, d, seed):
    """The NQ_MAX queries of a case group (the fixture stores them in full)."""
    xq = float_rand(NQ_MAX * d, seed).reshape(NQ_MAX, d) + np.float32(shift(kind))
    if kind == "ip":
        xq[NOHIT_QUERY] = 0.0          # every inner product is 0
    else:
        xq[NOHIT_QUERY] += np.float32(10.0)  # far from every row
    return np.ascontiguousarray(xq, np.float32)


def make_base(float_rand, kind, d, seed, xq):
    xb = float_rand(NB * d, seed).reshape(NB, d) + np.float32(shift(kind))
    k = np.arange(1, CLUSTER_ROWS.size + 1, dtype=np.float32)[:, None]
    q = xq[CLUSTER_QUERY][None, :]
    if kind == "offset":
        xb[CLUSTER_ROWS] = q + k * np.float32(2.0 ** -12)
        xb[EQUAL_ROWS] = xq[EQUAL_QUERIES]
    else:
        xb[CLUSTER_ROWS] = q * (np.float32(1.0) + k * np.float32(2.0 ** -10))
    return np.ascontiguousarray(xb, np.float32)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_flat_range.npz")
CASES = [f"{kind}_d{d}_nq{nq}" for kind in ("l2", "ip") for d in (13, 40, 128)
         for nq in (37, 19)] + ["bnd_l2", "bnd_ip", "cancel_l2"]


# File layout (few, concatenated arrays: an .npz entry costs ~130 bytes of
# headers however small it is):
#   groups, group_kind, group_sha256 [G]; group_meta [G, 4] = rows, d, seed,
#   metric_l2; xq = the groups' NQ_MAX x d queries, flattened, in group order;
#   cases [C]; case_group [C] (index into groups), case_nq, case_radius [C];
#   lims = the cases' nq + 1 limits, D / I (uint16 row numbers) = their
#   results, all in case order.
def case_arrays(gold, tag):
    """(group index, nq, radius, (lims, D, I)) of a fixture case."""
    c = [str(t) for t in gold["cases"]].index(tag)
    nqs = gold["case_nq"].astype(np.int64)
    l0 = int((nqs[:c] + 1).sum())
    all_lims = gold["lims"].astype(np.int64)
    lims = all_lims[l0:l0 + int(nqs[c]) + 1]
    # a case's results start where the totals of the cases before it end
    starts = np.cumsum(nqs + 1) - 1
    r0 = int(all_lims[starts[:c]].sum())
    D = gold["D"][r0:r0 + int(lims[-1])]
    I = gold["I"][r0:r0 + int(lims[-1])].astype(np.int64)
    return int(gold["case_group"][c]), int(nqs[c]), float(gold["case_radius"][c]), (lims, D, I)


def load_case(gold, orc, tag):
    """(xq, xb, metric_l2, radius, (lims, D, I)) of a fixture case; the
    database is rebuilt from its stream and checked against the stored hash."""
    g, nq, radius, want = case_arrays(gold, tag)
    meta = gold["group_meta"].astype(np.int64)
    nb, d, seed, ml2 = (int(v) for v in meta[g])
    assert nb == NB
    x0 = NQ_MAX * int(meta[:g, 1].sum())
    xq_all = gold["xq"][x0:x0 + NQ_MAX * d].reshape(NQ_MAX, d)
    xb = make_base(orc.float_rand, str(gold["group_kind"][g]), d, seed, xq_all)
    assert sha256(xb) == str(gold["group_sha256"][g])
    return np.ascontiguousarray(xq_all[:nq]), xb, bool(ml2), radius, want


def distance_matrix(orc, xq, xb, metric_l2, blas_form, member=None, per_pair=True):
    """[nq, nb] fp32 distances in the form the reference takes; NaN where the
    pair is not evaluated (non-members) or can never be a hit.  BLAS form: the
    distances of orc.knn(k = nb) scattered by id (the restatement
    tests/test_flat_range_fixtures.py pins against the reference); direct form:
    fvec_L2sqr / fvec_inner_product per pair over the members, or
    (per_pair=False, no selector, for the larger shapes) the same functions
    through orc.knn(blas_form=False)."""
    nq, nb = xq.shape[0], xb.shape[0]
    full = np.full((nq, nb), np.nan, np.float32)
    if nb == 0 or nq == 0:
        return full
    if blas_form or not per_pair:
        assert member is None
        D, I = orc.knn(xq, xb, nb, metric=1 if metric_l2 else 0, blas_form=blas_form)
        for i in range(nq):
            ok = I[i] >= 0
            full[i, I[i][ok]] = D[i][ok]
    else:
        f = orc.fvec_L2sqr if metric_l2 else orc.fvec_inner_product
        rows = range(nb) if member is None else np.nonzero(member)[0].tolist()
        for i in range(nq):
            for j in rows:
                full[i, j] = f(xq[i], xb[j])
    return full


def threshold(full, metric_l2, radius):
    """(lims, D, I) of a distance matrix: strict comparison, ascending rows."""
    r = np.float32(radius)
    with np.errstate(invalid="ignore"):
        hit = (full < r) if metric_l2 else (full > r)
    lims = np.zeros(full.shape[0] + 1, np.int64)
    lims[1:] = np.cumsum(hit.sum(axis=1))
    qi, I = np.nonzero(hit)       # row-major: query-major, rows ascending
    return lims, full[qi, I].astype(np.float32), I.astype(np.int64)


def restate(orc, xq, xb, metric_l2, radius, sel_member=None, per_pair=True):
    """IndexFlat::range_search: a selector or fewer than 20 queries take the
    direct form, anything else the BLAS form."""
    blas = sel_member is None and xq.shape[0] >= 20
    return threshold(distance_matrix(orc, xq, xb, metric_l2, blas, sel_member, per_pair),
                     metric_l2, radius)


def check_equal(got, want):
    lg, Dg, Ig = got
    lw, Dw, Iw = want
    assert np.array_equal(np.asarray(lg, np.int64), np.asarray(lw, np.int64)), \
        f"lims differ: totals {int(lg[-1])} vs {int(lw[-1])}"
    assert np.array_equal(np.asarray(Ig, np.int64), np.asarray(Iw, np.int64))
    # bit for bit (also tells -0.0 from 0.0 and compares NaN payload-free)
    assert np.array_equal(np.asarray(Dg, np.float32).view(np.uint32),
                          np.asarray(Dw, np.float32).view(np.uint32))
