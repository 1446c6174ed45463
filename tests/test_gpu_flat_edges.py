"""IndexFlat's fp32 path and the k-NN merges at their edge shapes.

Every other parity test leans on the exact IndexFlat search; this file gives
it a suite of its own.  The reference throughout is the oracle (orc.knn,
orc.merge_knn_results: one heap per query in arrival order), and ids AND
distances must be bit-equal: no tolerance appears anywhere.

  A  k_pairwise / flat_tile_contract at d below 4, just past a 32-dim chunk
     and above 128, row and query counts around the 128-wide tile, both
     forms (direct below 20 queries, BLAS form from 20), rows in ~3 copies so
     that the k boundary ties (inner product then needs select_fix_ip);
  B  k_select_rows' 512-candidate cap: the best columns laid out in one lane,
     the pass-2 count asserted from a numpy model before the search;
  C  more than 2^20 rows: the chunked select + merge (L2) and the whole-row
     path (inner product, k > 64), with ties across the chunk boundaries;
  D  k > 64 from IndexFlat at small sizes: LDS and global-scratch select,
     k > ntotal, the empty index, boundary ties, padding;
  E  the device merges k_merge_shards (k <= 64) and k_merge_general (k > 64):
     tie order, inner product, -1-ended shard rows, 256 shards, argument checks.

Where a case must run a particular path it asserts the stage name the library
records; every tie or cap condition is asserted from the oracle or the model
inside the test.
"""
import numpy as np
import pytest
import torch

import flat_edges_data as fd
from conftest import assert_same_results

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
TILE_SELECT = "flat_distance+select"        # fp32 tile + wave select
ROW_SELECT = "flat_distance+select_exact"   # whole rows + exact select


def ran_stages(amd, idx, fn):
    amd.set_kernel_timing(True)
    try:
        idx.reset_kernel_times()
        out = fn()
        names = {nm for nm, _, _ in idx.kernel_times()}
    finally:
        amd.set_kernel_timing(False)
    return out, names


def flat_index(amd, xb, metric):
    idx = amd.IndexFlat(xb.shape[1], metric)
    if xb.shape[0]:
        idx.add(xb)
    return idx


def assert_padding(D, I, nvalid, metric):
    pad = FLT_MAX if metric == 1 else -FLT_MAX
    assert (I[:, :nvalid] >= 0).all()
    assert (I[:, nvalid:] == -1).all() and (D[:, nvalid:] == pad).all()


# ---------------------------------------------------------------- A
# (d, ny, nq, k, data): every d of {1, 3, 4, 31, 32, 33, 36, 65, 132, 260},
# ny of {1, 63, 128, 129, 300}, nq of {20, 127, 128, 129, 257} and k of
# {1, 10, 64}; d = 33, 132, 260 each with a ragged ny and a ragged nq
TILE_CASES = [
    (1, 300, 129, 10, "signed"),
    (1, 63, 128, 64, "uniform"),      # k > ny
    (3, 129, 128, 1, "uniform"),
    (3, 300, 257, 10, "signed"),
    (4, 128, 127, 64, "signed"),
    (4, 1, 127, 10, "uniform"),       # k > ny
    (31, 63, 257, 10, "uniform"),
    (31, 128, 20, 1, "signed"),
    (32, 128, 128, 64, "signed"),
    (32, 129, 129, 10, "uniform"),
    (33, 129, 129, 10, "signed"),
    (33, 300, 257, 64, "uniform"),
    (36, 63, 20, 1, "signed"),
    (36, 300, 127, 10, "uniform"),
    (65, 129, 257, 64, "signed"),
    (65, 1, 20, 10, "uniform"),       # k > ny
    (132, 129, 129, 10, "signed"),
    (132, 300, 127, 1, "uniform"),
    (132, 63, 257, 64, "signed"),     # k > ny
    (260, 300, 129, 10, "uniform"),
    (260, 129, 257, 64, "signed"),
    (260, 1, 20, 1, "signed"),
]


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("d,ny,nq,k,kind", TILE_CASES)
def test_tile_and_dimension_edges(amd, orc, gpu, monkeypatch, d, ny, nq, k, kind, metric):
    xb = fd.rows_with_copies(kind, ny, d, 100 + d)
    xq = fd.queries_for(kind, xb, nq, 200 + d)
    if kind == "signed":
        assert (xb < 0).any() and (xb > 0).any()
    Dr, Ir = orc.knn(xq, xb, k, metric=metric, blas_form=True)
    if k < ny:
        tied = fd.boundary_ties(orc, xq, xb, k, metric)
        assert tied.mean() >= 0.25, tied.mean()
        if metric == 0:
            # the lexicographic choice of the wave select is not the heap's:
            # without select_fix_ip this case fails
            lex = fd.lex_topk(fd.distance_rows(orc, xq, xb, metric), k, metric)
            assert (np.sort(lex, axis=1) != np.sort(Ir, axis=1)).any()
    if d <= 128:
        monkeypatch.setenv("FAISS_AMD_COARSE", "f32")
    idx = flat_index(amd, xb, metric)
    (D, I), names = ran_stages(amd, idx, lambda: idx.search(xq, k))
    assert names == {TILE_SELECT}, names
    assert_same_results(D, I, Dr, Ir)
    if k > ny:
        assert_padding(D, I, ny, metric)


@pytest.mark.parametrize("metric", [1, 0])
def test_direct_form_below_20_queries(amd, orc, gpu, monkeypatch, metric):
    """19 queries take the direct form (fvec_L2sqr / fvec_inner_product per
    pair), 20 the BLAS form, on the same data; the two forms differ in at
    least one distance bit, so each run is told from the other."""
    d, ny, k = 36, 300, 10
    xb = fd.rows_with_copies("signed", ny, d, 31)
    xq = fd.queries_for("signed", xb, 20, 32)
    Dd, Id = orc.knn(xq[:19], xb, k, metric=metric, blas_form=False)
    Db, Ib = orc.knn(xq, xb, k, metric=metric, blas_form=True)
    assert (Dd.view(np.uint32) != Db[:19].view(np.uint32)).any()
    monkeypatch.setenv("FAISS_AMD_COARSE", "f32")
    idx = flat_index(amd, xb, metric)
    (D, I), names = ran_stages(amd, idx, lambda: idx.search(xq[:19].copy(), k))
    assert names == {TILE_SELECT}, names
    assert_same_results(D, I, Dd, Id)
    D, I = idx.search(xq, k)
    assert_same_results(D, I, Db, Ib)


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("k", [2, 10, 64])
@pytest.mark.parametrize("m", [511, 512, 600])
def test_select_candidate_cap(amd, orc, gpu, monkeypatch, m, k, metric):
    """Random data leaves pass 2 of k_select_rows with 1-3 k candidates: the
    lane minima are spread evenly, so T0 sits near the k-th best column.  With
    the m best columns in one lane, that lane contributes one minimum and T0
    is the (k-1)-th best of the far columns: pass 2 keeps all m and about k - 1
    more.  m = 511 at k = 2 gives 512, the last count the LDS buffer holds;
    m = 512 gives 513 and the whole-row sweep."""
    xb, xq, cluster = fd.cap_data(metric, m, 6)
    aimed = np.array(fd.CAP_AIMED)
    rows = fd.distance_rows(orc, xq, xb, metric)
    best = np.argsort(rows[aimed], axis=1, kind="stable")
    best = best[:, :m] if metric == 1 else best[:, -m:]
    assert (np.sort(best, axis=1) == cluster).all()      # the cluster is the top m
    top = rows[aimed].argmin(axis=1) if metric == 1 else rows[aimed].argmax(axis=1)
    assert (top == cluster[-1]).all()                    # its last row the single best
    if metric == 1:
        assert (rows[np.ix_(aimed, cluster)] < 0.01).all()
    passing = fd.select_pass2(rows, k, metric)
    counts = np.array([p.size for p in passing])
    fits = m == 511 and k == 2
    if k == 2:
        assert (counts[aimed] == m + 1).all(), counts[aimed]
    if fits:
        assert (counts <= fd.SEL_CAP).all() and (counts[aimed] == fd.SEL_CAP).all()
    else:
        assert (counts[aimed] > fd.SEL_CAP).all(), counts[aimed]
        # a select that stopped at its cap would lose the best row
        assert all(cluster[-1] in passing[q][fd.SEL_CAP:] for q in aimed)
    if not fits and k < 64:
        # rows 0-3 are one work group: two overflow, two do not.  (At k = 64
        # T0 is the worst lane minimum, lane 5's, whose columns are nearly all
        # cluster rows and far from the other queries: those overflow too.)
        assert (counts[:4] > fd.SEL_CAP).tolist() == [False, True, True, False], counts[:4]
    tied = fd.boundary_ties(orc, xq, xb, k, metric)
    if metric == 1:
        assert tied[aimed].all()
    else:
        # tied rows go on to select_fix_ip, which would mend a wrong select:
        # every other aimed query is tied, the rest stand on the select alone
        # (two values may still meet in fp32: at most one of the three)
        assert tied[aimed[::2]].all() and tied[aimed[1::2]].sum() <= 1
    monkeypatch.setenv("FAISS_AMD_COARSE", "f32")
    idx = flat_index(amd, xb, metric)
    (D, I), names = ran_stages(amd, idx, lambda: idx.search(xq, k))
    assert names == {TILE_SELECT}, names
    Dr, Ir = orc.knn(xq, xb, k, metric=metric, blas_form=True)
    assert_same_results(D, I, Dr, Ir)


# ---------------------------------------------------------------- C
CHUNK_SIZES = [fd.CHUNK + 1061, 2 * fd.CHUNK + 37]   # two chunks, three chunks


@pytest.fixture(scope="module")
def chunked(amd, gpu):
    """(ny, metric) -> (index, xb, hot rows), built once and kept."""
    cache = {}

    def get(ny, metric):
        if ny not in cache:
            xb, hot = cache[ny] = fd.chunk_data(ny, 9)
            assert (xb[fd.CHUNK - 1] == hot[0]).all() and (xb[fd.CHUNK] == hot[0]).all()
            for h in (0, 5, 11, 19):     # among those the queries use
                pos = np.nonzero((xb == hot[h]).all(axis=1))[0]
                assert 3 <= pos.size <= 42
                assert set((pos // fd.CHUNK).tolist()) == set(range(-(-ny // fd.CHUNK)))
        xb, hot = cache[ny]
        if (ny, metric) not in cache:
            cache[ny, metric] = flat_index(amd, xb, metric)
        return cache[ny, metric], xb, hot
    return get


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("k", [1, 5, 64, 100])
@pytest.mark.parametrize("nq", [40, 7])
@pytest.mark.parametrize("ny", CHUNK_SIZES)
def test_more_than_2_20_rows(amd, orc, chunked, ny, nq, k, metric):
    """L2 up to k = 64 runs the per-chunk select and the merge; inner product
    (whose arrival-order tie rule the chunks cannot restore) and k = 100 run the
    whole-row path.  40 queries take the BLAS form, 7 the direct form."""
    idx, xb, hot = chunked(ny, metric)
    xq = fd.chunk_queries(hot, nq, 3)
    blas = nq >= 20
    tied, across = fd.ties_across_chunks(orc, xq, xb, k, metric, blas)
    assert tied.mean() >= 0.25, tied.mean()
    if k <= 5 or ny > 2 * fd.CHUNK:
        # the tied rows lie in several chunks, so the chunks' order decides.
        # (The second chunk of the smaller index is 1061 rows: past the hot
        # rows' copies it rarely holds a member of a tied group.)
        assert across.mean() >= 0.25, across.mean()
    Dr, Ir = orc.knn(xq, xb, k, metric=metric, blas_form=blas)
    (D, I), names = ran_stages(amd, idx, lambda: idx.search(xq, k))
    assert names == {TILE_SELECT if metric == 1 and k <= 64 else ROW_SELECT}, names
    assert_same_results(D, I, Dr, Ir)


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("nq", [7, 40])
@pytest.mark.parametrize("ny,k", [(300, 2048), (2500, 65), (2500, 2048), (2500, 2049),
                                  (5000, 4096), (5, 100), (0, 100)])
def test_large_k_small_index(amd, orc, gpu, ny, k, nq, metric):
    """The whole-row path from IndexFlat: collection arrays in LDS up to
    k = 2048 and in global scratch beyond, k above and below ntotal, the empty
    index; rows in ~3 copies so that the boundary ties."""
    d = 12
    xb = fd.rows_with_copies("signed", ny, d, 41)
    xq = fd.queries_for("signed", xb, nq, 42)
    blas = nq >= 20
    if k < ny:
        tied = fd.boundary_ties(orc, xq, xb, k, metric, blas_form=blas)
        assert tied.mean() >= 0.25, tied.mean()
    Dr, Ir = orc.knn(xq, xb, k, metric=metric, blas_form=blas)
    idx = flat_index(amd, xb, metric)
    (D, I), names = ran_stages(amd, idx, lambda: idx.search(xq, k))
    assert names == {ROW_SELECT}, names
    assert_same_results(D, I, Dr, Ir)
    assert_padding(D, I, min(ny, k), metric)


# ---------------------------------------------------------------- E
def device_merge(amd, Dall, Iall, metric):
    """amd.merge_knn_results_device on torch device tensors."""
    ns, n, k = Dall.shape
    dev = torch.device("cuda:0")
    Dd = torch.from_numpy(Dall).to(dev)
    Id = torch.from_numpy(Iall).to(dev)
    Do = torch.empty((n, k), dtype=torch.float32, device=dev)
    Io = torch.empty((n, k), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    amd.merge_knn_results_device(n, k, ns, Dd.data_ptr(), Id.data_ptr(), Do.data_ptr(),
                                 Io.data_ptr(), metric)
    torch.cuda.synchronize(dev)
    return Do.cpu().numpy(), Io.cpu().numpy()


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("k", [1, 10, 64, 65, 300, 2048])
@pytest.mark.parametrize("ns", [1, 2, 5, 256])
def test_device_merges(amd, orc, gpu, ns, k, metric):
    """k <= 64 runs k_merge_shards, above it k_merge_general; n = 203 is ragged
    against their 4 and 64 queries per work group.  On a tie the lower shard
    comes first for L2 and the higher shard first for inner product."""
    n = 203
    Dall, Iall, nvalid = fd.shard_tables(ns, n, k, metric, 7)
    a, b = Dall[:, :, :-1], Dall[:, :, 1:]
    assert (a <= b).all() if metric == 1 else (a >= b).all()   # best first
    neg = Iall < 0
    assert (np.where(neg.any(axis=2), neg.argmax(axis=2), k) == nvalid).all()
    assert (nvalid == 0).any() and (nvalid == k).any()         # empty and full shard rows
    if k > 1:
        assert ((nvalid > 0) & (nvalid < k)).any()
    Dr, Ir = orc.merge_knn_results(Dall, Iall, metric)
    if ns > 1:
        ties = fd.cross_shard_tie_rows(Dall, nvalid, Dr, Ir, metric)
        assert ties.mean() >= 0.5, ties.mean()
    D, I = device_merge(amd, Dall, Iall, metric)
    assert_same_results(D, I, Dr, Ir)


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("k", [10, 65])
def test_device_merges_every_shard_empty(amd, orc, gpu, k, metric):
    Dall, Iall, nvalid = fd.shard_tables(5, 203, k, metric, 8, empty=True)
    assert not nvalid.any() and (Iall[:, :, 0] == -1).all()
    Dr, Ir = orc.merge_knn_results(Dall, Iall, metric)
    D, I = device_merge(amd, Dall, Iall, metric)
    assert_same_results(D, I, Dr, Ir)
    assert_padding(D, I, 0, metric)


@pytest.mark.parametrize("ns,k", [(257, 65), (1, 2049)])
def test_device_merge_argument_checks(amd, gpu, ns, k):
    """More shards than k_merge_general's position table holds, or a k above
    the exact path's limit, is an error, not a launch."""
    Dall = np.zeros((ns, 1, k), np.float32)
    Iall = np.zeros((ns, 1, k), np.int64)
    with pytest.raises(amd.FaissError):
        device_merge(amd, Dall, Iall, 1)
