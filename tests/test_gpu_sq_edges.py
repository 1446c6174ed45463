"""The IVF-SQ scan kernel (csrc/kernels_sq.hip, k_ex_sq) at the shapes and
flags the recorded reference runs of test_gpu_sq.py do not reach.

  * Parity with the reference on tests/golden/ref_sq_edges*
    (scripts/make_golden_sq_edges.py): by_residual off and on, SQfp16 with
    inner product, d = 8 / 24 / 72 / 264, lists of 0 / 1 / 255 / 256 / 257 /
    513 rows, a -1 probe, a list named twice, clamped codes, vdiff == 0,
    non-finite halves, ties at the k-th place, store_pairs, max_codes and a
    selector.
  * A wider grid against the numpy model (tests/sq_model.py, pinned to every
    recorded reference array by test_sq_model.py): qtype x metric x
    by_residual at d = 8 .. 520 (d > 256: a second trip of the LDS staging
    loop) over lists of up to 769 rows (a third pass of the row loop).
  * k = 2048 (kMaxKExact) below and above the row count, the k = 2049 error.
  * The 2^20-entry launch split and the 1 GiB query-chunk split with SQ's own
    offsets (e0, cdis + q0 np, lim + q0 np).
  * Repeated searches, scratch regrowth and the device entry point.
Ids and distances are compared bit for bit.

The exact path serves k <= 2048, so where a reference run has k = 2 nb > 2048
the kernel runs with k = 2048 and is compared with the first 2048 columns: no
query of the fixtures scans more than 1795 rows, so both results hold every
admitted row in the same order and the columns beyond are padding (asserted).
For the same reason the grid (2755 rows) compares every row's arithmetic
through two searches that split the lists between them, beside the top 2048
of all of them."""
import os

import numpy as np
import pytest

import sq_edges_data as sd
import sq_model as sm
from conftest import assert_same_results, device_search

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
KMAX = 2048
F32 = np.float32


@pytest.fixture(scope="module")
def ex():
    return np.load(os.path.join(GOLD, "ref_sq_edges.npz"))


@pytest.fixture(scope="module")
def edge_indexes(amd, gpu):
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = amd.read_index(os.path.join(GOLD, "ref_sq_edges", tag + ".faiss"))
        return cache[tag]
    return get


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("tag", sd.TAGS)
def test_edges_search_preassigned(edge_indexes, ex, tag):
    idx = edge_indexes(tag)
    nb = int(ex[f"{tag}_meta"][2])
    xq, keys, cdis = ex[f"{tag}_xq"], ex[f"{tag}_keys"], ex[f"{tag}_cdis"]
    idx.nprobe = idx.nlist
    for k in (1, 10, 600, 2 * nb):
        Dr, Ir = ex[f"{tag}_pre_{k}_D"], ex[f"{tag}_pre_{k}_I"].astype(np.int64)
        if k > KMAX:
            assert (Ir[:, KMAX - 1:] == -1).all()  # fewer than 2048 rows admitted
            Dr, Ir = Dr[:, :KMAX], Ir[:, :KMAX]
        D, I = idx.search_preassigned(xq, min(k, KMAX), keys, cdis)
        assert_same_results(D, I, Dr, Ir)


@pytest.mark.parametrize("tag", sd.PARAM_TAGS)
def test_edges_store_pairs(edge_indexes, ex, tag):
    idx = edge_indexes(tag)
    idx.nprobe = idx.nlist
    D, I = idx.search_preassigned(ex[f"{tag}_xq"], 10, ex[f"{tag}_keys"], ex[f"{tag}_cdis"],
                                  store_pairs=True)
    assert_same_results(D, I, ex[f"{tag}_sp_10_D"], ex[f"{tag}_sp_10_I"])


@pytest.mark.parametrize("tag", sd.PARAM_TAGS)
def test_edges_max_codes_and_selector(amd, edge_indexes, ex, tag):
    """IndexIVF::search with parameters: this library's own coarse quantizer
    must find the reference's probes, then max_codes cuts a list inside the
    first row pass (1), at its end (256), one row later (257) and inside the
    second (300)"""
    idx = edge_indexes(tag)
    xq, nlist = ex[f"{tag}_xq"], idx.nlist
    sel = amd.IDSelectorBatch(np.sort(ex[f"{tag}_ids"].astype(np.int64))[::2])
    runs = [(f"mc{mc}", dict(max_codes=mc)) for mc in sd.MAX_CODES]
    runs += [("sel", dict(sel=sel)), ("mc300_sel", dict(max_codes=300, sel=sel))]
    for name, kw in runs:
        D, I = idx.search(xq, 10, params=amd.SearchParametersIVF(nprobe=nlist, **kw))
        assert_same_results(D, I, ex[f"{tag}_params_{name}_D"],
                            ex[f"{tag}_params_{name}_I"].astype(np.int64))


# ---------------------------------------------------------------- grid
LENS = [0, 1, 63, 64, 65, 255, 256, 257, 512, 513, 769]
VARIANTS = [(qt, l2, br) for qt in (sm.QT_8bit, sm.QT_fp16) for l2 in (1, 0) for br in (1, 0)]
DIMS = [8, 16, 24, 40, 72, 136, 264, 520]


def vid(v):
    return ("sq8" if v[0] == sm.QT_8bit else "fp16") + ("_l2" if v[1] else "_ip") + \
           ("_res" if v[2] else "_nores")


def build(amd, orc, qtype, l2, br, d, lens, seed):
    """An index with lists of the given lengths, trained and filled here; the
    last tenth of every list repeats its first rows under other ids."""
    nlist = len(lens)
    lists = np.repeat(np.arange(nlist, dtype=np.int64), lens)
    nb = lists.size
    cent = ((orc.float_rand(nlist * d, seed).reshape(nlist, d) - F32(0.5)) * F32(2)).astype(F32)
    xb = (cent[lists] + F32(0.6) * (orc.float_rand(nb * d, seed + 1).reshape(nb, d) - F32(0.5)))
    xb = xb.astype(F32)
    off = np.concatenate([[0], np.cumsum(lens)])
    for l, n in enumerate(lens):
        if n // 10:
            xb[off[l + 1] - n // 10:off[l + 1]] = xb[off[l]:off[l] + n // 10]
    ids = np.random.RandomState(seed).permutation(nb).astype(np.int64) * 5 + 1
    q = amd.IndexFlatL2(d) if l2 else amd.IndexFlatIP(d)
    q.add(cent)
    idx = amd.IndexIVFScalarQuantizer(q, d, nlist, qtype,
                                      amd.METRIC_L2 if l2 else amd.METRIC_INNER_PRODUCT,
                                      by_residual=bool(br))
    xt = xb[::2].copy()  # ranges from every second row, dimension 1 constant
    xt[:, 1] = F32(0.25)
    idx.train(xt)
    idx.add_core(xb, ids, lists)
    assert [idx.get_list_size(l) for l in range(nlist)] == list(lens)
    return idx, xb, ids, lists


def queries(orc, nq, d, nlist, seed):
    xq = ((orc.float_rand(nq * d, seed).reshape(nq, d) - F32(0.5)) * F32(2)).astype(F32)
    cdis = (orc.float_rand(nq * nlist, seed + 1).reshape(nq, nlist) - F32(0.5)).astype(F32)
    rs = np.random.RandomState(seed)
    keys = np.stack([np.arange(nlist), np.arange(nlist)[::-1]] +
                    [rs.permutation(nlist) for _ in range(nq - 2)]).astype(np.int64)
    return xq, keys, cdis


@pytest.fixture(scope="module")
def grid(amd, orc, gpu):
    cache = {}

    def get(v, d):
        if (v, d) not in cache:
            idx, xb, ids, lists = build(amd, orc, v[0], v[1], v[2], d, LENS, 9100 + d)
            cache[(v, d)] = (idx, sm.Model.from_index(idx), xb, lists)
        return cache[(v, d)]
    return get


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_grid_equals_model(grid, orc, v, d):
    idx, m, xb, lists = grid(v, d)
    assert (m.l2, m.by_residual, m.qtype) == (bool(v[1]), bool(v[2]), v[0])
    # the host encode
    codes = np.concatenate([idx.list_codes(l) for l in range(idx.nlist)])
    np.testing.assert_array_equal(codes, m.encode(xb, lists))
    nlist = idx.nlist
    xq, keys, cdis = queries(orc, 4, d, nlist, 9200 + d)
    idx.nprobe = nlist
    # the best 2048 of all 2755 rows
    D, I = idx.search_preassigned(xq, KMAX, keys, cdis)
    Dm, Im = m.search_preassigned(xq, KMAX, keys, cdis)
    assert (Im >= 0).all()
    assert_same_results(D, I, Dm, Im)
    # every row: the lists split between two searches, the other probes -1
    big = np.isin(keys, [nlist - 2, nlist - 1])
    for part, rows in ((big, sum(LENS[-2:])), (~big, sum(LENS[:-2]))):
        kp = np.where(part, keys, -1)
        D, I = idx.search_preassigned(xq, KMAX, kp, cdis)
        Dm, Im = m.search_preassigned(xq, KMAX, kp, cdis)
        assert ((Im >= 0).sum(axis=1) == rows).all() and rows < KMAX
        assert_same_results(D, I, Dm, Im)


# ---------------------------------------------------------------- k edges
def test_k_2048_and_2049(amd, grid, edge_indexes, ex, orc):
    # fewer rows than k: every row, then padding
    tag = "sq8_l2_d8"
    idx = edge_indexes(tag)
    m = sm.Model.from_index(idx)
    xq, keys, cdis = ex[f"{tag}_xq"], ex[f"{tag}_keys"], ex[f"{tag}_cdis"]
    idx.nprobe = idx.nlist
    D, I = idx.search_preassigned(xq, KMAX, keys, cdis)
    Dm, Im = m.search_preassigned(xq, KMAX, keys, cdis)
    assert (Im[:, -1] == -1).all() and (Dm[:, -1] == np.finfo(F32).max).all()
    assert_same_results(D, I, Dm, Im)
    # more rows than k, through search() on the index's own probes
    v, d = (sm.QT_fp16, 0, 1), 24
    idx, m, _, _ = grid(v, d)
    xq, _, _ = queries(orc, 4, d, idx.nlist, 9300)
    idx.nprobe = idx.nlist
    D, I = idx.search(xq, KMAX)
    Dq, Iq = idx.quantizer.search(xq, idx.nlist)
    Dm, Im = m.search_preassigned(xq, KMAX, Iq, Dq)
    assert (Im >= 0).all() and idx.ntotal > KMAX
    assert_same_results(D, I, Dm, Im)
    with pytest.raises(amd.FaissError, match="2048"):
        idx.search(xq, KMAX + 1)
    with pytest.raises(amd.FaissError, match="2048"):
        idx.search_preassigned(xq, KMAX + 1, Iq, Dq)


# ---------------------------------------------------------------- splits
@pytest.fixture(scope="module")
def split_indexes(amd, orc, gpu):
    cache = {}

    def get(v, lens, seed):
        if (v, seed) not in cache:
            idx, _, _, _ = build(amd, orc, v[0], v[1], v[2], 8, lens, seed)
            cache[(v, seed)] = (idx, sm.Model.from_index(idx))
        return cache[(v, seed)]
    return get


@pytest.mark.parametrize("period", [64, 60])
@pytest.mark.parametrize("v", [(sm.QT_8bit, 1, 1), (sm.QT_fp16, 0, 1)], ids=vid)
def test_launch_split(split_indexes, orc, v, period):
    """16400 x 64 (query, probe) entries: the scan's second launch starts at
    entry 2^20, query 16384 (e = e0 + blockIdx.x).  The queries repeat with
    period 64; with period 60 query 16384 is not the query the first launch
    began with, so values read without e0 differ too."""
    nlist, d, nq = 64, 8, 16400
    assert nq * nlist > 1 << 20 and (1 << 20) % nlist == 0
    idx, m = split_indexes(v, [2] * nlist, 9400)
    xq, _, cdis = queries(orc, period, d, nlist, 9401)
    keys = np.stack([np.roll(np.arange(nlist, dtype=np.int64), q) for q in range(period)])
    Dm, Im = m.search_preassigned(xq, 10, keys, cdis)
    rep = np.arange(nq) % period
    idx.nprobe = nlist
    D, I = idx.search_preassigned(xq[rep], 10, keys[rep], cdis[rep])
    assert_same_results(D, I, Dm[rep], Im[rep])


@pytest.mark.parametrize("period", [8, 7])
def test_query_chunk_split(amd, split_indexes, orc, period):
    """Inner product by residual with a list of 8192 rows and nprobe = 32: a
    query's candidate slot is 32 x 8192 rows, so the 1 GiB key budget holds 512
    queries and queries 512..519 run in a second chunk that reads the coarse
    distances and max_codes limits at q0 np.  The queries repeat with period 8;
    with period 7 query 512 is not query 0 again, so a chunk that read them
    without q0 np would return other values."""
    nlist, d, nq = 32, 8, 520
    idx, m = split_indexes((sm.QT_8bit, 0, 1), [8192] + [4] * (nlist - 1), 9500)
    xq, _, _ = queries(orc, period, d, nlist, 9501)
    rep = np.arange(nq) % period
    # the probes of the whole batch (from 20 queries on the flat quantizer takes
    # its matrix-product form, whose coarse distances the search adds)
    Dq, Iq = idx.quantizer.search(xq[rep], nlist)
    assert np.array_equal(Dq, Dq[rep]) and np.array_equal(Iq, Iq[rep])
    Dm, Im = m.search_preassigned(xq, 10, Iq[:period], Dq[:period], max_codes=9000)
    D, I = idx.search(xq[rep], 10, params=amd.SearchParametersIVF(nprobe=nlist, max_codes=9000))
    assert_same_results(D, I, Dm[rep], Im[rep])


# ---------------------------------------------------------------- repeats
def test_repeat_regrow_and_device_entry(grid, orc):
    v, d = (sm.QT_8bit, 1, 1), 72
    idx, m, _, _ = grid(v, d)
    xq, _, _ = queries(orc, 4, d, idx.nlist, 9600)
    idx.nprobe = idx.nlist
    first = idx.search(xq, 10)
    second = idx.search(xq, 10)
    idx.search(xq, KMAX)  # a larger k in between
    third = idx.search(xq, 10)
    fourth = device_search(idx, xq, 10)
    for D, I in (second, third, fourth):
        assert_same_results(D, I, *first)
    Dq, Iq = idx.quantizer.search(xq, idx.nlist)
    assert_same_results(*first, *m.search_preassigned(xq, 10, Iq, Dq))
