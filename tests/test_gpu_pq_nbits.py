"""IndexIVFPQ with 4- to 7-bit codes on the GPU.

Against the reference: tests/golden/ref_pq_nbits.npz and the index files in
tests/golden/ref_pq_nbits/ (scripts/make_golden_pq_nbits.py; every k = 10 query
has a group of 8 bit-equal distances cut by the boundary, under shuffled ids).
Ids and distances must be equal bit for bit on the default path (the
list-centric LDS-table scan, csrc/kernels_pq_lut.hip, where it is eligible) and
with FAISS_AMD_PQ_SCAN=exact (the general exact scan, csrc/kernels_exact.hip).

Against the model (tests/pq_nbits_model.py, pinned to the same reference
results by tests/test_pq_nbits_model.py): small indexes built on a fixture's
codebook that walk the scan's edges.  The scan's constants: QT = 64 queries per
work item, QI = 4 queries per table pass, k <= 64 eligible."""
import os

import numpy as np
import pytest

import pq_nbits_model as pm
from conftest import assert_same_results, device_search

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ref_pq_nbits")
TAGS = ["PQ16x4", "PQ10x5", "PQ32x6", "PQ24x7", "PQ16x4_ip"]
QT, QI, KMAX = 64, 4, 64
MODES = ["default", "exact"]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_pq_nbits.npz"))


def load(amd, tag):
    return amd.read_index(os.path.join(GOLD, tag + ".faiss"))


@pytest.fixture(scope="module")
def indexes(amd, gpu):
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = load(amd, tag)
            cache[tag].nprobe = 4
        return cache[tag]
    return get


def queries(orc, fx, tag):
    d, seed = int(fx[f"{tag}_meta"][0]), int(fx[f"{tag}_meta"][6])
    return orc.float_rand(32 * d, seed + 2).reshape(32, d)


def rows(orc, fx, tag):
    """(xb, ids) the generator added: 250 base rows 8 times, shuffled ids."""
    d, seed = int(fx[f"{tag}_meta"][0]), int(fx[f"{tag}_meta"][6])
    xb = np.ascontiguousarray(np.tile(orc.float_rand(250 * d, seed + 1).reshape(250, d), (8, 1)))
    return xb, np.random.RandomState(seed + 3).permutation(2000).astype(np.int64)


def set_mode(monkeypatch, mode):
    if mode == "exact":
        monkeypatch.setenv("FAISS_AMD_PQ_SCAN", "exact")
    else:
        monkeypatch.delenv("FAISS_AMD_PQ_SCAN", raising=False)


def set_table(idx, tag, table):
    if not tag.endswith("_ip"):
        idx.use_precomputed_table = table


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", TAGS)
def test_search_equals_reference(indexes, fx, orc, monkeypatch, tag, mode):
    set_mode(monkeypatch, mode)
    idx = indexes(tag)
    xq = queries(orc, fx, tag)
    keys, cdis = fx[f"{tag}_Iq"].astype(np.int64), fx[f"{tag}_Dq"]
    for t in fx[f"{tag}_tables"]:
        table = max(int(t), 0)
        set_table(idx, tag, table)
        for k in fx[f"{tag}_ks"]:
            k = int(k)
            want = fx[f"{tag}_t{table}_{k}_D"], fx[f"{tag}_t{table}_{k}_I"].astype(np.int64)
            assert_same_results(*idx.search_preassigned(xq, k, keys, cdis), *want)
            assert_same_results(*idx.search(xq, k), *want)
            assert_same_results(*device_search(idx, xq, k), *want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,table", [("PQ16x4", 1), ("PQ16x4", 0), ("PQ16x4_ip", 0)])
def test_range_equals_reference(indexes, fx, orc, monkeypatch, tag, table, mode):
    set_mode(monkeypatch, mode)
    idx = indexes(tag)
    set_table(idx, tag, table)
    tt = f"{tag}_t{table}"
    lims, D, I = idx.range_search(queries(orc, fx, tag), float(fx[f"{tt}_radius"]))
    assert np.array_equal(lims, fx[f"{tt}_range_lims"])
    assert np.array_equal(I, fx[f"{tt}_range_I"])
    assert np.array_equal(D, fx[f"{tt}_range_D"])
    lims2, D2, I2 = idx.range_search_preassigned(queries(orc, fx, tag), float(fx[f"{tt}_radius"]),
                                                 fx[f"{tag}_Iq"], fx[f"{tag}_Dq"])
    assert np.array_equal(lims2, lims) and np.array_equal(I2, I) and np.array_equal(D2, D)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("table", [1, 0])
def test_max_codes_selector_equals_reference(amd, indexes, fx, orc, monkeypatch, table, mode):
    set_mode(monkeypatch, mode)
    idx = indexes("PQ16x4")
    idx.use_precomputed_table = table
    sel = amd.IDSelectorBatch(np.arange(0, 2000, 3))
    params = amd.SearchParametersIVF(nprobe=4, max_codes=150, sel=sel)
    D, I = idx.search(queries(orc, fx, "PQ16x4"), 10, params=params)
    assert_same_results(D, I, fx[f"PQ16x4_t{table}_params_D"],
                        fx[f"PQ16x4_t{table}_params_I"].astype(np.int64))


@pytest.mark.parametrize("tag", TAGS)
def test_add_equals_reference_lists(amd, indexes, fx, orc, tag):
    """encode_vectors + add on the trained, emptied index: every list's codes
    and ids as the reference holds them."""
    idx = amd.clone_index(indexes(tag))
    idx.reset()
    assert idx.ntotal == 0 and idx.is_trained
    xb, ids = rows(orc, fx, tag)
    idx.add_with_ids(xb[:700], ids[:700])
    idx.add_with_ids(xb[700:], ids[700:])
    sizes = fx[f"{tag}_list_sizes"]
    off = np.concatenate([[0], np.cumsum(sizes)])
    for l in range(idx.nlist):
        assert np.array_equal(idx.list_ids(l), fx[f"{tag}_list_ids"][off[l]:off[l + 1]]), l
        assert np.array_equal(idx.list_codes(l), fx[f"{tag}_list_codes"][off[l]:off[l + 1]]), l


def test_encode_equals_reference_codes(amd, indexes, fx, orc):
    idx = amd.clone_index(indexes("PQ16x4"))
    idx.reset()
    xb, _ = rows(orc, fx, "PQ16x4")
    idx.add(xb[:64])  # ids 0..63
    where = {}
    for l in range(idx.nlist):
        for j, i in enumerate(idx.list_ids(l)):
            where[int(i)] = (l, j)
    codes = {l: idx.list_codes(l) for l in range(idx.nlist)}
    for i in range(64):
        l, j = where[i]
        assert l == fx["PQ16x4_enc_list"][i]
        assert np.array_equal(codes[l][j], fx["PQ16x4_enc_codes"][i]), i


def assert_same_up_to_tie_order(D, I, D0, I0):
    """Bit-equal distances; the same ids for every distance value above the
    row's last one (whose group the k boundary may cut): the same id where the
    value occurs once, the same set of ids where it is tied."""
    assert np.array_equal(D, D0)
    for q in range(len(D)):
        for v in np.unique(D0[q]):
            at = D0[q] == v
            if v != D0[q, -1]:
                assert sorted(I[q][at]) == sorted(I0[q][at]), (q, v)


@pytest.mark.parametrize("shard_type", [1, 2, 4])
def test_shards_equal_unsharded(amd, indexes, fx, orc, shard_type):
    """The PQ16x4 index over 2000 distinct rows: the sharded result equals the
    unsharded one, ids and distances, for every query whose unsharded top k + 1
    holds no two equal distances (rows with equal codes in one list tie bit for
    bit even here, rarely; nearly every query must be free of that).

    The fixture's own content is groups of 8 copies.  The shards' merge
    (merge_knn_results) takes bit-equal distances in shard order, the unsharded
    heap in arrival order, so the order inside a tied group, and which of its
    members survive at the k boundary, differ by construction (in the reference
    as well); there everything else must be equal."""
    src = indexes("PQ16x4")
    src.use_precomputed_table = 1
    xq = queries(orc, fx, "PQ16x4")
    distinct = amd.clone_index(src)
    distinct.reset()
    distinct.add(orc.float_rand(2000 * 64, 4501).reshape(2000, 64))
    distinct.nprobe = 4
    sh = amd.index_ivf_to_shards(distinct, 3, shard_type, devices=[0, 0, 0])
    sh.nprobe = 4
    assert sh.ntotal == distinct.ntotal
    for k in (1, 10, 100):
        D1, _ = distinct.search(xq, k + 1)
        free = np.array([len(np.unique(row)) == k + 1 for row in D1])
        # a tie needs two of ~125 rows of a list to share a 64-bit code: at
        # least three quarters of the queries must be compared in full
        assert free.sum() >= 24, (k, int(free.sum()))
        (D, I), (D0, I0) = sh.search(xq, k), distinct.search(xq, k)
        assert np.array_equal(D, D0)
        assert np.array_equal(I[free], I0[free])
    sh = amd.index_ivf_to_shards(src, 3, shard_type, devices=[0, 0, 0])
    sh.nprobe = 4
    assert sh.ntotal == src.ntotal
    for k in (1, 10, 100):
        assert_same_up_to_tie_order(*sh.search(xq, k), *src.search(xq, k))
    # the copies of one base row are what ties: slot by slot the same base row
    _, ids = rows(orc, fx, "PQ16x4")
    row_of = np.empty(2000, np.int64)
    row_of[ids] = np.arange(2000)
    for k in (1, 10):
        assert np.array_equal(row_of[sh.search(xq, k)[1]] % 250, row_of[src.search(xq, k)[1]] % 250)


def test_refine_over_low_bit_base(amd, gpu, orc):
    d, nb = 64, 4000
    xb = orc.float_rand(nb * d, 4401).reshape(nb, d)
    xq = orc.float_rand(40 * d, 4402).reshape(40, d)
    idx = amd.index_factory(d, "IVF16,PQ16x4,RFlat")
    idx.train(xb)
    idx.add(xb)
    idx.k_factor = 8
    idx.base_index.nprobe = 8
    D, I = idx.search(xq, 10)
    for i in (0, 13, 39):
        for j in range(10):
            assert D[i, j] == np.float32(orc.fvec_L2sqr(xq[i], xb[I[i, j]]))
    _, Ib = idx.base_index.search(xq, 10)
    base_exact = np.array([[orc.fvec_L2sqr(xq[i], xb[j]) for j in Ib[i]] for i in range(40)])
    assert (D[:, -1] <= base_exact.max(axis=1)).all()


# ---------------------------------------------------------------- model
LENGTHS = [0, 1, 63, 64, 65, 300, 7, 130, 2, 31, 33, 5, 9, 17, 100, 257]


@pytest.fixture(scope="module", params=["PQ16x4", "PQ10x5"])
def small(request, amd, gpu, orc):
    """The fixture's trained index with lists of chosen lengths: random rows
    picked by the list the coarse quantizer gives them (a third of the rows of
    a list repeat an earlier row of it, so ties cross every boundary); ids
    shuffled."""
    tag = request.param
    idx = load(amd, tag)
    idx.reset()
    d = idx.d
    rng = np.random.RandomState(77)
    pool = orc.float_rand(12000 * d, 500).reshape(12000, d)
    _, lst = idx.quantizer.search(pool, 1)
    xs = []
    for l, n in enumerate(LENGTHS):
        x = pool[lst[:, 0] == l][:n].copy()
        assert len(x) == n, (l, len(x))
        for j in range(2, n, 3):
            x[j] = x[rng.randint(0, j)]
        xs.append(x)
    xb = np.concatenate(xs)
    idx.add_with_ids(xb, rng.permutation(len(xb)).astype(np.int64))
    got = [idx.get_list_size(l) for l in range(16)]
    assert got == LENGTHS, got
    return tag, idx


def model_of(tag, idx, cache={}):
    key = (tag, idx.use_precomputed_table)
    if key not in cache:
        cache[key] = pm.Model.from_index(idx)
    return cache[key]


def check(tag, idx, xq, k, keys, monkeypatch, with_cdis=True):
    """search_preassigned on both paths against the model."""
    cent = idx.quantizer.xb
    cdis = None
    if with_cdis:  # any fp32 values serve: table 1 adds them as dis0
        cdis = np.array([[((xq[i] - cent[max(l, 0)]) ** 2).sum() for l in keys[i]]
                         for i in range(len(xq))], np.float32)
    want = model_of(tag, idx).search_preassigned(xq, k, keys, cdis)
    idx.nprobe = keys.shape[1]
    for mode in MODES:
        set_mode(monkeypatch, mode)
        assert_same_results(*idx.search_preassigned(xq, k, keys, cdis), *want)


@pytest.mark.parametrize("table", [1, 0])
def test_list_lengths(small, orc, monkeypatch, table):
    tag, idx = small
    idx.use_precomputed_table = table
    d = idx.d
    nq = 24
    xq = idx.quantizer.xb[np.arange(nq) % 16] + 0.25 * orc.float_rand(nq * d, 611).reshape(nq, d)
    # every list is probed, the empty one (0) and the single-row one (1) first
    keys = np.array([[0, 1, (2 + i) % 16, (5 + 3 * i) % 16] for i in range(nq)], np.int64)
    for k in (1, 10):
        check(tag, idx, xq.astype(np.float32), k, keys, monkeypatch)


@pytest.mark.parametrize("per_list", [1, QI - 1, QI, QI + 1, QT + 1])
def test_queries_per_item(small, orc, monkeypatch, per_list):
    """per_list queries probe list 5 (300 rows) and nothing else shares it."""
    tag, idx = small
    idx.use_precomputed_table = 1
    d = idx.d
    nq = per_list + 3
    xq = (idx.quantizer.xb[5] + 0.3 * orc.float_rand(nq * d, 612).reshape(nq, d)).astype(np.float32)
    keys = np.full((nq, 2), -1, np.int64)
    keys[:per_list, 0] = 5
    keys[:, 1] = [2 + (i % 3) for i in range(nq)]  # lists 2, 3, 4 (63, 64, 65 rows)
    check(tag, idx, xq, 10, keys, monkeypatch)


def test_many_queries_few_lists(small, orc, monkeypatch):
    """nprobe 2 over 4 lists with 3 QT queries: items past QT queries per list."""
    tag, idx = small
    idx.use_precomputed_table = 1
    d = idx.d
    nq = 3 * QT
    rng = np.random.RandomState(9)
    lists = np.array([5, 7, 14, 15])
    xq = (idx.quantizer.xb[lists[np.arange(nq) % 4]] +
          0.3 * orc.float_rand(nq * d, 613).reshape(nq, d)).astype(np.float32)
    keys = np.array([rng.choice(lists, 2, replace=False) for _ in range(nq)], np.int64)
    check(tag, idx, xq, 10, keys, monkeypatch)


@pytest.mark.parametrize("k", [1, KMAX, KMAX + 1, 2048])
def test_k_edges(small, orc, monkeypatch, k):
    tag, idx = small
    idx.use_precomputed_table = 1
    d = idx.d
    nq = 6
    xq = (idx.quantizer.xb[[5, 7, 14, 15, 2, 3]] +
          0.3 * orc.float_rand(nq * d, 614).reshape(nq, d)).astype(np.float32)
    keys = np.array([[5, 7, 14], [7, 5, 15], [14, 15, 13], [15, 2, 3], [2, 0, 1], [3, 4, 5]],
                    np.int64)
    check(tag, idx, xq, k, keys, monkeypatch)


def test_nprobe_equals_nlist(small, orc, monkeypatch):
    tag, idx = small
    d = idx.d
    nq = 5
    xq = (idx.quantizer.xb[:nq] + 0.3 * orc.float_rand(nq * d, 615).reshape(nq, d)).astype(
        np.float32)
    keys = np.array([np.roll(np.arange(16), i) for i in range(nq)], np.int64)
    for table in (1, 0):
        idx.use_precomputed_table = table
        check(tag, idx, xq, 10, keys, monkeypatch)
    # through search(): the coarse quantizer orders all 16 lists
    idx.nprobe = 16
    want = None
    for mode in MODES:
        set_mode(monkeypatch, mode)
        got = idx.search(xq, 10)
        if want is not None:
            assert_same_results(*got, *want)
        want = got


def stage_names(amd, idx, run):
    amd.set_kernel_timing(True)
    try:
        idx.reset_kernel_times()
        run()
        return [name for name, ms, _ in idx.kernel_times() if ms > 0]
    finally:
        amd.set_kernel_timing(False)
        idx.reset_kernel_times()


def test_default_path_is_the_lut_scan(amd, indexes, fx, orc, monkeypatch):
    """The stage timers name the scan that ran: ivfpq_lut where eligible, the
    general scan past k = KMAX, when forced, and at 8 bits never the LUT scan."""
    idx = indexes("PQ16x4")
    xq = queries(orc, fx, "PQ16x4")
    set_mode(monkeypatch, "default")
    names = stage_names(amd, idx, lambda: idx.search(xq, 10))
    assert "ivfpq_lut" in names and "ivf_exact_scan" not in names
    names = stage_names(amd, idx, lambda: idx.search(xq, KMAX + 1))
    assert "ivf_exact_scan" in names and "ivfpq_lut" not in names
    set_mode(monkeypatch, "exact")
    names = stage_names(amd, idx, lambda: idx.search(xq, 10))
    assert "ivf_exact_scan" in names and "ivfpq_lut" not in names


def test_candidate_buffer_overflow(amd, gpu, orc, monkeypatch):
    """2200 copies of one row: every one of them lies under the bound, more than
    the candidate buffer (2048 per query) holds, and the scan resolves the query
    over all its probes; with an IDSelector that leaves fewer than k rows there is no bound
    at all."""
    idx = load(amd, "PQ16x4")
    idx.reset()
    pool = orc.float_rand(3000 * 64, 700).reshape(3000, 64)
    xb = np.concatenate([np.tile(pool[:1], (2200, 1)), pool[1:]])
    rng = np.random.RandomState(3)
    idx.add_with_ids(xb, rng.permutation(len(xb)).astype(np.int64))
    xq = np.ascontiguousarray(pool[:4] + np.float32(0.01))
    _, keys = idx.quantizer.search(xq, 4)
    idx.use_precomputed_table = 1
    for k in (1, 10, KMAX):
        check("overflow", idx, xq, k, keys, monkeypatch)
    idx.nprobe = 4
    few = amd.IDSelectorBatch(np.arange(5))
    params = amd.SearchParametersIVF(nprobe=4, sel=few)
    got = {}
    for mode in MODES:
        set_mode(monkeypatch, mode)
        got[mode] = idx.search(xq, 10, params=params)
    assert_same_results(*got["default"], *got["exact"])
    assert (got["default"][1] < 5).all() and (got["default"][1] == -1).any()


def test_search_stats_and_counters(amd, indexes, fx, orc, monkeypatch):
    set_mode(monkeypatch, "default")
    idx = indexes("PQ16x4")
    idx.use_precomputed_table = 1
    xq = queries(orc, fx, "PQ16x4")
    D, I, st = idx.search_stats(xq, 10)
    assert_same_results(D, I, fx["PQ16x4_t1_10_D"], fx["PQ16x4_t1_10_I"].astype(np.int64))
    assert (st["list_scan_us"] > 0).all() and (st["total_us"] >= st["list_scan_us"]).all()
    stats = amd.cvar.indexIVF_stats
    stats.reset()
    idx.search(xq, 10)
    sizes = fx["PQ16x4_list_sizes"]
    assert stats.nq == 32 and stats.nlist == 32 * 4
    assert stats.ndis == int(sizes[fx["PQ16x4_Iq"]].sum())


def test_seven_bit_codes_on_the_lut_scan(amd, gpu, orc, monkeypatch):
    """PQ16x7 at d 64 (16 x 128 entries: inside the LDS-table scan's budget, which
    the PQ24x7 fixture is not), trained here: both scans against the model of the
    trained index, a third of the rows repeating an earlier one."""
    d, nb = 64, 1500
    xb = orc.float_rand(nb * d, 7701).reshape(nb, d).copy()
    rng = np.random.RandomState(11)
    for j in range(2, nb, 3):
        xb[j] = xb[rng.randint(0, j)]
    idx = amd.index_factory(d, "IVF16,PQ16x7")
    idx.train(orc.float_rand(4000 * d, 7702).reshape(4000, d))
    idx.add_with_ids(xb, rng.permutation(nb).astype(np.int64))
    assert idx.code_size == 14 and idx.pq_info()["nbits"] == 7
    xq = orc.float_rand(12 * d, 7703).reshape(12, d)
    _, keys = idx.quantizer.search(xq, 5)
    for table in (1, 0):
        idx.use_precomputed_table = table
        check(f"PQ16x7_t{table}", idx, xq, 10, keys, monkeypatch)
    set_mode(monkeypatch, "default")
    idx.nprobe = 5
    assert "ivfpq_lut" in stage_names(amd, idx, lambda: idx.search(xq, 10))


def test_not_by_residual(amd, gpu, fx, orc, monkeypatch, tmp_path):
    """by_residual = false has no setter in the binding: the PQ16x4 fixture file
    with that byte cleared (the u8 before code_size, d, M, nbits).  The codes
    then stand for the rows themselves; the table is the query's own and dis0
    is 0.  Both scans against the model."""
    import struct
    raw = bytearray(open(os.path.join(GOLD, "PQ16x4.faiss"), "rb").read())
    pat = b"\x01" + struct.pack("<QQQQ", 8, 64, 16, 4)
    at = raw.find(pat)
    assert at > 0 and raw.find(pat, at + 1) < 0
    raw[at] = 0
    f = tmp_path / "nores.faiss"
    f.write_bytes(bytes(raw))
    idx = amd.read_index(f)
    info = idx.pq_info()
    assert info["by_residual"] is False and info["use_precomputed_table"] == 0
    xq = queries(orc, fx, "PQ16x4")[:12]
    keys = fx["PQ16x4_Iq"][:12].astype(np.int64)
    for k in (1, 10):
        check("PQ16x4_nores", idx, xq, k, keys, monkeypatch)
    set_mode(monkeypatch, "default")
    assert "ivfpq_lut" in stage_names(amd, idx, lambda: idx.search(xq, 10))
