"""Inputs and helpers shared by scripts/make_golden_pq_filter.py,
tests/test_ref_pq_filter.py and tests/test_gpu_pq_filter_edges.py: the 8-bit
IVF-PQ geometries the bf16 MFMA filter (kernels_pq_mfma.hip k_ivfpq_filter_w)
is instantiated for, the inputs of the reference-run fixtures
tests/golden/ref_pq_filter*, oracle views of a subset of an index, and the
planted data sets of the re-rank's rare paths.

`float_rand(n, seed)` is the reference's generator (oracle.float_rand).
"""
import re

import numpy as np

# every (d, M) the filter serves: dsub 2, 4, 8 at d = 64, 96, 128
GEOMS = [(64, 32), (64, 16), (64, 8), (96, 48), (96, 24), (96, 12), (128, 64), (128, 32),
         (128, 16)]

# ---------------------------------------------------------------- reference-run fixtures
# the four geometries tests/golden/ref_full does not hold
REF_TAGS = {"pq_m32d64": (64, 32), "pq_m12d96": (96, 12), "pq_m64d128": (128, 64),
            "pq_m16d128": (128, 16)}
REF_NLIST, REF_NT, REF_NB, REF_NQ = 16, 6000, 2000, 64
REF_NREP, REF_COPIES = 16, 25
REF_CASES = [(16, 1), (16, 10), (16, 20), (5, 10)]  # (nprobe, k) of search_preassigned
REF_PARAMS = dict(nprobe=8, max_codes=300, k=10)     # the one SearchParametersIVF call


def ref_inputs(float_rand, tag):
    """Training rows, base rows, ids, queries and selector ids of one tag.

    2000 base rows: 1600 distinct ones and 16 vectors 25 times each, in a
    fixed shuffled order, so equal codes meet inside the lists and a k below
    25 cuts a group of equal distances.  The ids are a permutation (times 3,
    plus 7), so id order is not arrival order.  Half of the 64 queries are
    copies of the repeated vectors."""
    d, M = REF_TAGS[tag]
    seed = 7000 + d + M
    xt = float_rand(REF_NT * d, seed).reshape(REF_NT, d)
    ndist = REF_NB - REF_NREP * REF_COPIES
    rep = xt[ndist:ndist + REF_NREP]
    rows = np.concatenate([xt[:ndist], np.repeat(rep, REF_COPIES, axis=0)])
    xb = np.ascontiguousarray(rows[np.random.RandomState(seed).permutation(REF_NB)])
    ids = np.random.RandomState(seed + 1).permutation(REF_NB).astype(np.int64) * 3 + 7
    xq = np.ascontiguousarray(np.concatenate(
        [rep, rep, float_rand((REF_NQ - 2 * REF_NREP) * d, seed + 2).reshape(-1, d)]))
    sel = np.sort(ids[np.random.RandomState(seed + 3).random_sample(REF_NB) < 0.4])
    return dict(d=d, M=M, xt=xt, xb=xb, ids=ids, xq=xq, sel=np.ascontiguousarray(sel))


# ---------------------------------------------------------------- oracle views
def oracle_of_rows(orc, idx, off, codes, ids):
    """An IVFOracle over the given lists with idx's quantizer and codebooks."""
    info = idx.pq_info()
    pq = dict(M=info["M"], nbits=info["nbits"], by_residual=info["by_residual"],
              centroids=idx.pq_centroids)
    return orc.IVFOracle(idx.d, idx.nlist, idx.metric_type, off, codes, ids, idx.quantizer.xb,
                         None, pq)


def subset_oracle(orc, idx, sel_ids):
    """The oracle over the member rows only, list order kept: what a search
    with an IDSelector must return (the reference's tests/test_search_params.py
    compares with such a subset index)."""
    off, codes, ids = idx.invlists_arrays()
    keep = np.isin(ids, sel_ids)
    noff = np.zeros_like(off)
    noff[1:] = np.cumsum([int(keep[off[l]:off[l + 1]].sum()) for l in range(idx.nlist)])
    return oracle_of_rows(orc, idx, noff, codes[keep], ids[keep])


def oracle_params_search(orc, idx, xq, k, keys, cdis, max_codes, sel_ids, table):
    """search_preassigned with max_codes and an IDSelector as IndexIVF.cpp:
    445-460, 546-550 and 609-622 have it: a query walks its probes in coarse
    order, a list counts with all its rows (members or not) towards max_codes,
    the list that reaches the cap is cut to the rows still allowed and the
    later ones are not scanned; of the scanned rows only the members enter the
    heap.  One oracle per query over exactly the rows it may scan."""
    off, codes, ids = idx.invlists_arrays()
    member = np.isin(ids, sel_ids) if sel_ids is not None else np.ones(ids.shape, bool)
    n = xq.shape[0]
    D = np.empty((n, k), np.float32)
    I = np.empty((n, k), np.int64)
    for q in range(n):
        take = np.zeros(idx.nlist, np.int64)
        nscan = 0
        for l in keys[q]:
            if l < 0:
                continue
            ln = int(off[l + 1] - off[l])
            if max_codes > 0:
                ln = min(ln, max_codes - nscan)
            take[l] = ln  # (a list named twice would be scanned twice: not in these inputs)
            nscan += ln
            if max_codes > 0 and nscan >= max_codes:
                break
        rows = np.concatenate([np.arange(off[l], off[l] + take[l]) for l in range(idx.nlist)])
        rows = rows[member[rows]].astype(np.int64)
        noff = np.searchsorted(rows, off).astype(np.int64)
        ref = oracle_of_rows(orc, idx, noff, codes[rows], ids[rows])
        ref.use_precomputed_table = table
        D[q], I[q] = (a[0] for a in ref.search_preassigned(xq[q:q + 1], k, keys[q:q + 1],
                                                           cdis[q:q + 1]))
    return D, I


# ---------------------------------------------------------------- GPU-side helpers
def ran_stages(amd, idx, fn):
    """fn() with kernel timing on: (its result, the names of the stages that ran)."""
    amd.set_kernel_timing(True)
    try:
        idx.reset_kernel_times()
        out = fn()
        names = {nm for nm, _, _ in idx.kernel_times()}
    finally:
        amd.set_kernel_timing(False)
    return out, names


def assert_filter_ran(names):
    assert "ivfpq_filter" in names and "ivfpq_rerank" in names, names
    assert "ivf_exact_scan" not in names, names


STATS_RE = re.compile(r"ivfpq mfma scan: nq=(\d+) survivors/q=([0-9.]+) exact rows/q=([0-9.]+) "
                      r"failing streams/q=([0-9.]+) overflow queries=(\d+) "
                      r"general-resolve queries=(\d+)")


def scan_stats(err):
    """The counters of the last `ivfpq mfma scan:` line (FAISS_AMD_IVF_STATS=1)."""
    m = STATS_RE.findall(err)
    assert m, err[-400:]
    nq, surv, rows, fail, over, gen = m[-1]
    return dict(nq=int(nq), survivors=float(surv), exact_rows=float(rows), failing=float(fail),
                overflow=int(over), general=int(gen))


def filled_ivfpq(amd, cent, M, train, xb, ids=None):
    """IndexIVFPQ over the given centroids (a filled flat quantizer is not
    trained again), the PQ trained on `train`'s residuals."""
    d = cent.shape[1]
    quant = amd.IndexFlatL2(d)
    quant.add(np.ascontiguousarray(cent, np.float32))
    idx = amd.IndexIVFPQ(quant, d, cent.shape[0], M)
    idx.train(np.ascontiguousarray(train, np.float32))
    xb = np.ascontiguousarray(xb, np.float32)
    if ids is None:
        ids = permuted_ids(xb.shape[0])
    idx.add_with_ids(xb, ids)
    return idx


def permuted_ids(n, seed=17):
    """ids whose order is not the arrival order (a sort by (distance, id), up
    or down, then differs from the reference's arrival-order rule at a tie)"""
    return np.random.RandomState(seed).permutation(n).astype(np.int64) * 5 + 3


# ---- planted sets of the re-rank's rare paths, d = 64
RR_D = 64
LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, 256]
COUNT_SIZES = [64, 65, 128, 256, 257, 512, 513]


def exact_lengths_set(float_rand, d):
    """16 far-apart centroids, list l = LENGTHS[l] rows next to centroid l."""
    cent = np.ascontiguousarray(10.0 * float_rand(16 * d, 5315).reshape(16, d))
    noise = float_rand(sum(LENGTHS) * d, 5316).reshape(-1, d)
    xb = np.ascontiguousarray(np.repeat(cent, LENGTHS, axis=0) + 0.05 * noise)
    xq = np.ascontiguousarray(5.0 * float_rand(129 * d, 5317).reshape(129, d))
    return cent, xb, xq


def ties_set(float_rand):
    """80 vectors 25 times each, shuffled; 32 of them and 32 random queries.
    Trained on the 80 vectors and 1920 random rows (the PQ needs 256 points)."""
    d = RR_D
    base = float_rand(80 * d, 5301).reshape(80, d)
    perm = np.random.RandomState(3).permutation(80 * 25)
    xb = np.ascontiguousarray(np.repeat(base, 25, axis=0)[perm])
    train = np.ascontiguousarray(np.concatenate([base, float_rand(1920 * d, 5303).reshape(-1, d)]))
    xq = np.ascontiguousarray(np.concatenate([base[:32], float_rand(32 * d, 5302).reshape(32, d)]))
    return train, xb, xq


def uncertifiable_set(float_rand, big_rows=600, copies=False):
    """15 lists of 20 rows and one of `big_rows` rows within 1e-3 of its
    centroid (copies: that many copies of one vector there).  32 queries
    beside the big list and 32 random ones.  The PQ is trained on the
    spread-out form of the rows in either case."""
    d = RR_D
    cent = float_rand(16 * d, 5306).reshape(16, d)
    rng = np.random.RandomState(9)
    small = np.repeat(cent[:15], 20, axis=0) + 0.02 * rng.standard_normal((300, d))
    spread = cent[15] + 1e-3 * rng.standard_normal((big_rows, d))
    train = np.concatenate([small, spread]).astype(np.float32)
    big = np.repeat(spread[:1], big_rows, axis=0) if copies else spread
    xb = np.concatenate([small, big]).astype(np.float32)
    xq = np.concatenate([cent[15] + 1e-3 * rng.standard_normal((32, d)),
                         float_rand(32 * d, 5307).reshape(32, d)]).astype(np.float32)
    return cent, np.ascontiguousarray(train), np.ascontiguousarray(xb), np.ascontiguousarray(xq)


def candidate_count_set(float_rand):
    """List i holds COUNT_SIZES[i] copies of one vector beside its centroid;
    the centroids are far apart (orthogonal directions, norm 4); three more
    lists hold 12 copies each.  Four queries beside each sized list."""
    d, nl = RR_D, len(COUNT_SIZES) + 3
    cent = np.zeros((nl, d), np.float32)
    cent[np.arange(nl), np.arange(nl)] = 4.0
    cent += float_rand(nl * d, 5308).reshape(nl, d) * np.float32(0.01)
    rng = np.random.RandomState(13)
    v = (cent + 0.01 * rng.standard_normal((nl, d))).astype(np.float32)
    sizes = COUNT_SIZES + [12, 12, 12]
    xb = np.ascontiguousarray(np.repeat(v, sizes, axis=0))
    train = (np.repeat(cent, 40, axis=0) + 0.01 * rng.standard_normal((40 * nl, d))).astype(np.float32)
    nq = 4 * len(COUNT_SIZES)
    xq = (np.repeat(v[:len(COUNT_SIZES)], 4, axis=0) + 0.01 * rng.standard_normal((nq, d)))
    return cent, np.ascontiguousarray(train), xb, np.ascontiguousarray(xq.astype(np.float32))
