"""Inputs and small numpy models for tests/test_gpu_flat_edges.py.

    rows_with_copies(kind, ny, d, seed)   database whose rows come in ~3 copies
    queries_for(kind, xb, nq, seed)       queries, a few of them database rows
    distance_rows(orc, xq, xb, metric, blas_form)
                                          the oracle's full [nq, ny] distances
    lex_topk(rows, k, metric)             the lexicographic top-k of wave_select.h
    boundary_ties(orc, xq, xb, k, ...)    queries whose k-th distance == (k+1)-th
    select_pass2(rows, k, metric)         pass 1 / pass 2 of k_select_rows
    cap_data(metric, m, seed)             section B: the best m columns in one lane
    chunk_data(ny, seed)                  section C: > 2^20 rows with ties
    ties_across_chunks(orc, xq, xb, k, ...)  ... and whether they span chunks
    shard_tables(ns, n, k, metric, seed)  section E: sorted, tied, -1-ended rows
"""
import numpy as np

import hard_data

SEL_LANES = 64   # k_select_rows: one wave per row, column c belongs to lane c % 64
SEL_CAP = 512    # its LDS candidate buffer


def rows_with_copies(kind, ny, d, seed):
    """ny rows drawn from ceil(ny / 3) distinct ones, the copies scattered:
    every distance of a row occurs about three times, so the k-th and the
    (k+1)-th best tie for most queries whatever k is."""
    if ny == 0:
        return np.empty((0, d), np.float32)
    nbase = (ny + 2) // 3
    base = hard_data.make(kind, nbase, d, seed)
    perm = np.random.default_rng([seed, 77]).permutation(ny)
    return np.ascontiguousarray(base[perm % nbase])


def queries_for(kind, xb, nq, seed):
    """Queries of the database's distribution; every fifth one is a database
    row (L2 distance 0 against each of its copies: the clamp at 0)."""
    ny, d = xb.shape
    xq = hard_data.make(kind, nq, d, seed + 7919)
    if ny:
        for i in range(0, nq, 5):
            xq[i] = xb[(13 * i + 1) % ny]
    return np.ascontiguousarray(xq)


def distance_rows(orc, xq, xb, metric, blas_form=True):
    """The oracle's whole distance rows [nq, ny] (its k = ny result scattered
    back by label; every value here is admissible, so none is dropped)."""
    ny = xb.shape[0]
    D, I = orc.knn(xq, xb, ny, metric=metric, blas_form=blas_form)
    assert (I >= 0).all()
    rows = np.empty_like(D)
    np.put_along_axis(rows, I, D, axis=1)
    return rows


def _keys(rows, metric):
    """wave_select.h to_key: L2 (dis, id), inner product (-ip, -id)."""
    ids = np.arange(rows.shape[1], dtype=np.int64)
    return (rows, ids) if metric == 1 else (-rows, -ids)


def lex_topk(rows, k, metric):
    """Labels of the k smallest (key1, key2) per row: what the wave select
    returns before select_fix_ip looks at it."""
    k1, k2 = _keys(rows, metric)
    return np.stack([np.lexsort((k2, r))[:k] for r in k1])


def boundary_ties(orc, xq, xb, k, metric, blas_form=True):
    """Per query: does the oracle's k-th distance equal its (k+1)-th?"""
    D, I = orc.knn(xq, xb, k + 1, metric=metric, blas_form=blas_form)
    return (I[:, k] >= 0) & (D[:, k - 1] == D[:, k])


def select_pass2(rows, k, metric):
    """k_select_rows on distance rows [nq, ny]: pass 1 keeps each lane's
    minimum (key, id) over its strided columns, T0 is the k-th smallest lane
    minimum, pass 2 compacts the columns with (key, id) <= T0 in column order.
    Returns those columns per row; more than SEL_CAP of them and the kernel
    takes its whole-row sweep (its buffer holds the first SEL_CAP)."""
    out = []
    keys, k2 = _keys(rows, metric)
    for k1 in keys:
        mins = []
        for lane in range(min(SEL_LANES, k1.size)):
            a, b = k1[lane::SEL_LANES], k2[lane::SEL_LANES]
            j = np.lexsort((b, a))[0]
            mins.append((a[j], b[j]))
        mins.sort()
        if len(mins) < k:          # fewer than k lanes hold a column: T0 = +inf
            out.append(np.arange(k1.size))
            continue
        t1, t2 = mins[k - 1]
        out.append(np.nonzero((k1 < t1) | ((k1 == t1) & (k2 <= t2)))[0])
    return out


# ---------------------------------------------------------------- section B
CAP_D = 8
CAP_NQ = 24
CAP_AIMED = (1, 2, 7, 9, 14, 20, 23)   # rows 1 and 2 share a work group with 0 and 3
CAP_LANE = 5


def cap_data(metric, m, seed):
    """d = 8, ny just above 64 m.  Rows 64 i + 5 (i < m), all in lane 5 of the
    select, are the best of every aimed query: within 0.01 of it for L2, a
    large multiple of it for inner product.  They cycle through 37 distinct
    vectors, so their distances tie exactly and the k-th best ties with the
    next one (inner product: for every other aimed query, see below); the last
    of them is the single best.  All other rows are far away (unit normal)."""
    rng = np.random.default_rng([seed, m, metric])
    d, ny = CAP_D, 64 * m + 37
    xb = rng.standard_normal((ny, d)).astype(np.float32)
    c = (rng.choice([-1.0, 1.0], d) * rng.uniform(6.0, 8.0, d)).astype(np.float32)
    noise = rng.uniform(-0.03, 0.03, (37, d)).astype(np.float32)
    scale = np.float32(1.0 if metric == 1 else 50.0)
    cluster = 64 * np.arange(m) + CAP_LANE
    xb[cluster] = scale * c + noise[np.arange(m) % 37]
    # the very best row is the last of them: a select that drops the
    # candidates past its cap loses it
    xb[cluster[-1]] = (scale + np.float32(0.0 if metric == 1 else 0.5)) * c
    xq = rng.standard_normal((CAP_NQ, d)).astype(np.float32)
    if metric != 1:
        # away from the cluster's direction: its rows are these queries' worst
        flip = (xq @ c) > 0
        xq[flip] = -xq[flip]
    for i, q in enumerate(CAP_AIMED):
        xq[q] = c + rng.uniform(-0.001, 0.001, d).astype(np.float32)
    if metric != 1:
        # A boundary tie sends an inner-product row through select_fix_ip, which
        # selects it again from the whole row whatever k_select_rows answered.
        # So only every other aimed query sees ties: the cluster rows differ in
        # their last coordinate, which those queries have at exactly 0.
        xb[cluster[:-1], d - 1] += rng.uniform(-2.0, 2.0, m - 1).astype(np.float32)
        xq[list(CAP_AIMED[::2]), d - 1] = 0.0
    return xb, xq, cluster


# ---------------------------------------------------------------- section C
CHUNK = 1 << 20
CHUNK_D = 4
CHUNK_HOT = 64


def chunk_data(ny, seed):
    """d = 4.  Rows are random on a signed grid of 16 levels per coordinate
    (65536 distinct rows, each met ~16-32 times), so a query's distances tie
    in groups at every rank, k = 64 and 100 included.  64 hot rows, off the
    grid, are each copied to 3-40 distinct positions, one of them in every
    2^20-row chunk (a short last chunk takes the first hot rows only, which are
    the ones chunk_queries uses); hot row 0 also sits at rows 2^20 - 1 and
    2^20.  Returns (xb, hot)."""
    rng = np.random.default_rng([seed, ny])
    xb = (rng.integers(-8, 8, (ny, CHUNK_D)).astype(np.float32) / np.float32(8.0))
    hot = rng.standard_normal((CHUNK_HOT, CHUNK_D)).astype(np.float32)
    nchunk = -(-ny // CHUNK)
    perm = rng.permutation(ny)
    perm = perm[(perm != CHUNK - 1) & (perm != CHUNK)]
    by_chunk = [perm[perm // CHUNK == c] for c in range(nchunk)]
    spare = rng.permutation(np.concatenate([b[CHUNK_HOT:] for b in by_chunk]))
    used = 0
    for h in range(CHUNK_HOT):
        pos = [int(b[h]) for b in by_chunk if h < min(CHUNK_HOT, 2 * len(b) // 3)]
        extra = max(int(rng.integers(3, 41)) - len(pos), 0)
        pos += spare[used:used + extra].tolist()
        used += extra
        if h == 0:
            pos += [CHUNK - 1, CHUNK]
        xb[pos] = hot[h]
    return np.ascontiguousarray(xb), hot


def ties_across_chunks(orc, xq, xb, k, metric, blas_form):
    """Per query: (the k-th distance equals the (k+1)-th, rows of two or more
    chunks hold the k-th distance), read from the oracle's k + 64 best."""
    D, I = orc.knn(xq, xb, k + 64, metric=metric, blas_form=blas_form)
    tied = D[:, k - 1] == D[:, k]
    spans = np.array([len(set((i[d == d[k - 1]] // CHUNK).tolist())) > 1 for d, i in zip(D, I)])
    return tied, tied & spans


def chunk_queries(hot, nq, seed):
    """The hot rows, then as many random queries."""
    rng = np.random.default_rng([seed, nq, 1])
    nh = (nq + 1) // 2
    xq = rng.standard_normal((nq, CHUNK_D)).astype(np.float32)
    xq[:nh] = hot[:nh]
    return np.ascontiguousarray(xq)


# ---------------------------------------------------------------- section E
def shard_tables(ns, n, k, metric, seed, empty=False):
    """[ns, n, k] distances and labels as shards return them: integer-valued
    distances from a range of at most 50 (narrower when ns k is small, so that
    the shards' values still meet), each row best first (ascending for L2,
    descending for inner product); about a third of the rows end early at a
    label -1, some at position 0, half of them with stale labels behind the -1
    (a list ends at its first negative label).  empty: every row ends at 0.
    Returns (D, I, nvalid [ns, n]: the length of each row's list)."""
    rng = np.random.default_rng([seed, ns, n, k, metric])
    span = min(50, 1 + ns * k // 4)
    if ns * n * k <= (1 << 22):
        D = np.sort(rng.integers(0, span, (ns, n, k), dtype=np.int16), axis=2)
        I = rng.integers(0, 10 ** 6, (ns, n, k), dtype=np.int64)
    else:
        # (kept cheap) sorted by construction: a walk that climbs `span` over
        # the row, drawn for a seventh of the queries and repeated; the rows'
        # ends below still differ
        n0 = -(-n // 7)
        D = np.cumsum(rng.random((ns, n0, k), np.float32) < span / k, axis=2, dtype=np.int16)
        D = np.tile(D, (1, 7, 1))[:, :n]
        I = (np.arange(n * k, dtype=np.int64) * 7919 % 10 ** 6).reshape(1, n, k) \
            + 13 * np.arange(ns, dtype=np.int64).reshape(ns, 1, 1)
    D = D.astype(np.float32)
    D -= np.float32(span // 2)
    if metric != 1:
        np.negative(D, out=D)
    cut = rng.integers(0, k + 1, (ns, n))
    cut[rng.random((ns, n)) < 0.25] = 0
    ends = rng.random((ns, n)) < 0.35
    if empty:
        cut[:] = 0
        ends[:] = True
    ends &= cut < k
    s, r = np.nonzero(ends)
    I[s, r, cut[s, r]] = -1
    s, r = np.nonzero(ends & (rng.random((ns, n)) < 0.5))
    I[s, r] = np.where(np.arange(k) >= cut[s, r][:, None], -1, I[s, r])
    return D, I, np.where(ends, cut, k)


def cross_shard_tie_rows(Dall, nvalid, Dm, Im, metric):
    """Rows of the merge in which the shard order decides a label: a value
    at least as good as the k-th merged one is held, among the first 64 valid
    entries of their rows, by two or more shards."""
    ns, n, k = Dall.shape
    w = min(k, 64)
    sign = 1.0 if metric == 1 else -1.0
    key = sign * Dall[:, :, :w]
    nm = (Im >= 0).sum(axis=1)
    last = sign * Dm[np.arange(n), np.maximum(nm, 1) - 1]
    valid = np.arange(w) < nvalid[..., None]
    ok = valid & (key <= last[None, :, None]) & (nm > 0)[None, :, None]
    lo = key.min()
    v = (key - lo).astype(np.int64)
    R = int(v.max()) + 1
    pres = np.zeros((ns, n, R), bool)
    s, r, p = np.nonzero(ok)
    pres[s, r, v[s, r, p]] = True
    return (pres.sum(axis=0) >= 2).any(axis=1)
