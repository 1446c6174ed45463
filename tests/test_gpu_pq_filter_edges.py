"""The 8-bit IVF-PQ search path — the bf16 MFMA filter k_ivfpq_filter_w
(kernels_pq_mfma.hip) and the exact re-rank ivfpq_rerank_ds<2|4|8>
(ivf_rerank.h) — at its edge shapes, ids and distance bits against the oracle
(tests/test_ref_fixtures.py and tests/test_ref_pq_filter.py pin it to the
reference at all nine geometries) and against the reference-run fixtures
tests/golden/ref_pq_filter*.  No tolerances.

  a. all nine (d, M) instances x the 2, 4 and 8 key streams (k = 1, 10, 20,
     and nprobe < k), both precomputed-table settings, an IDSelector;
  b. query widths 1 .. 193 through one list's items (a second query half of
     one column, items of one query);
  c. lists of exactly 0 .. 256 rows;
  d. the task walk past two rounds of the grid, its schedules and group
     sizes, and the 4-wave work-group form (unfolded keys);
  e. the re-rank's rare paths: a k-th key tied for every query, failing
     streams, candidate overflow and the general resolve, candidate counts on
     both sides of every batch boundary;
  f. max_codes where the nearest rows lie in the cut-off part of a list.

Every test that means to reach the filter asserts that the ivfpq_filter and
ivfpq_rerank stages ran and ivf_exact_scan did not.
"""
import os

import numpy as np
import pytest
# imported before the library is loaded (the fixtures below load it): the two
# then share one HIP runtime, and torch can be asked for the CU count
import torch

import pq_filter_data as pf
from conftest import assert_same_results, rand

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GDIR = os.path.join(HERE, "golden", "ref_pq_filter")
FX = np.load(os.path.join(HERE, "golden", "ref_pq_filter.npz"))

NLIST = 16
NQMAX = 193
GEOM_IDS = [f"M{M}d{d}" for d, M in pf.GEOMS]
# (nprobe, k): the 2, 4 and 8 key streams, and nprobe < k (8 streams)
GRID = [(16, 1), (16, 10), (16, 20), (4, 10)]


class Geom:
    """IVF16,PQ<M>x8 over 3200 rand rows, trained by the library on them; 193
    queries; the oracle over the same index.  Oracle results are computed
    once per (table, nprobe, k) and shared."""

    def __init__(self, amd, orc, d, M):
        self.amd, self.orc, self.d, self.M = amd, orc, d, M
        xb = rand(orc, 3200, d, 5400 + d + M)
        self.xq = rand(orc, NQMAX, d, 5500 + d + M)
        idx = amd.index_factory(d, f"IVF{NLIST},PQ{M}x8")
        idx.train(xb)
        idx.add(xb)
        self.idx = idx
        self.ref = orc.IVFOracle.from_index(idx)
        self.memo = {}

    def expect(self, table, nprobe, k):
        key = (table, nprobe, k)
        if key not in self.memo:
            self.ref.use_precomputed_table = table
            self.memo[key] = self.ref.search(self.xq, k, nprobe, nslices=1)
        return self.memo[key]

    def check_search(self, table, nprobe, k, nq):
        """IndexIVF::search end to end on the first nq queries (nq >= 20: the
        coarse quantizer's BLAS form on both sides)."""
        Dr, Ir, _, _ = self.expect(table, nprobe, k)
        self.idx.use_precomputed_table = table
        self.idx.nprobe = nprobe
        xq = np.ascontiguousarray(self.xq[:nq])
        (D, I), names = pf.ran_stages(self.amd, self.idx, lambda: self.idx.search(xq, k))
        pf.assert_filter_ran(names)
        assert_same_results(D, I, Dr[:nq], Ir[:nq])

    def check_preassigned(self, table, nprobe, k, nq):
        """search_preassigned on the oracle's probes: any nq sees the same
        coarse keys and distances as the batch of 193."""
        Dr, Ir, CD, CI = self.expect(table, nprobe, k)
        self.idx.use_precomputed_table = table
        self.idx.nprobe = nprobe
        xq = np.ascontiguousarray(self.xq[:nq])
        (D, I), names = pf.ran_stages(
            self.amd, self.idx, lambda: self.idx.search_preassigned(xq, k, CI[:nq], CD[:nq]))
        pf.assert_filter_ran(names)
        assert_same_results(D, I, Dr[:nq], Ir[:nq])


@pytest.fixture(scope="module")
def geoms(amd, orc, gpu):
    made = {}

    def get(d, M):
        if (d, M) not in made:
            made[(d, M)] = Geom(amd, orc, d, M)
        return made[(d, M)]
    return get


# ---------------------------------------------------------------- a. geometry x streams
@pytest.mark.parametrize("nprobe,k", GRID)
@pytest.mark.parametrize("table", [1, 0])
@pytest.mark.parametrize("dM", pf.GEOMS, ids=GEOM_IDS)
def test_geometry_stream_grid(geoms, dM, table, nprobe, k):
    geoms(*dM).check_search(table, nprobe, k, 129)


@pytest.mark.parametrize("dM", pf.GEOMS, ids=GEOM_IDS)
def test_geometry_with_selector(amd, orc, geoms, dM):
    g = geoms(*dM)
    keep = np.nonzero(np.random.RandomState(3).random_sample(3200) < 0.4)[0].astype(np.int64)
    sub = pf.subset_oracle(orc, g.idx, keep)
    sub.use_precomputed_table = 1
    xq = np.ascontiguousarray(g.xq[:129])
    Dr, Ir, _, _ = sub.search(xq, 10, 8, nslices=1)
    g.idx.use_precomputed_table = 1
    sp = amd.SearchParametersIVF(nprobe=8, sel=amd.IDSelectorBatch(keep))
    (D, I), names = pf.ran_stages(amd, g.idx, lambda: g.idx.search(xq, 10, params=sp))
    pf.assert_filter_ran(names)
    assert_same_results(D, I, Dr, Ir)
    assert np.isin(I[I >= 0], keep).all()


@pytest.fixture(scope="module")
def ref_files(amd, gpu):
    return {tag: amd.read_index(os.path.join(GDIR, tag + ".faiss")) for tag in pf.REF_TAGS}


@pytest.mark.parametrize("table", [1, 0])
@pytest.mark.parametrize("tag", list(pf.REF_TAGS))
def test_reference_files_preassigned(amd, ref_files, tag, table):
    idx = ref_files[tag]
    xq = FX[tag + "_xq"]
    idx.use_precomputed_table = table
    for nprobe, k in pf.REF_CASES:
        idx.nprobe = nprobe
        (D, I), names = pf.ran_stages(amd, idx, lambda: idx.search_preassigned(
            xq, k, FX[f"{tag}_q{nprobe}_I"], FX[f"{tag}_q{nprobe}_D"]))
        pf.assert_filter_ran(names)
        key = f"{tag}_t{table}_pre_{nprobe}_{k}"
        assert_same_results(D, I, FX[key + "_D"], FX[key + "_I"])


@pytest.mark.parametrize("tag", list(pf.REF_TAGS))
def test_reference_files_max_codes_selector(amd, ref_files, tag):
    idx = ref_files[tag]
    idx.use_precomputed_table = 1
    pr = pf.REF_PARAMS
    sp = amd.SearchParametersIVF(nprobe=pr["nprobe"], max_codes=pr["max_codes"],
                                 sel=amd.IDSelectorBatch(FX[tag + "_params_sel"]))
    (D, I), names = pf.ran_stages(amd, idx,
                                  lambda: idx.search(FX[tag + "_xq"], pr["k"], params=sp))
    pf.assert_filter_ran(names)
    assert_same_results(D, I, FX[tag + "_params_D"], FX[tag + "_params_I"])


# ---------------------------------------------------------------- b. query widths
WIDTH_GEOMS = [(64, 16), (96, 12)]
WIDTH_IDS = ["M16d64", "M12d96"]


@pytest.mark.parametrize("nq", [1, 31, 32, 33, 63, 64, 65, 96, 97, 129, 193])
@pytest.mark.parametrize("dM", WIDTH_GEOMS, ids=WIDTH_IDS)
def test_query_widths(geoms, dM, nq):
    # nprobe = nlist: every list's items see exactly nq queries, split at 64;
    # a task is (item, query half of 32)
    geoms(*dM).check_preassigned(1, NLIST, 10, nq)


@pytest.mark.parametrize("k", [1, 20])
@pytest.mark.parametrize("nq", [1, 33, 65])
@pytest.mark.parametrize("dM", WIDTH_GEOMS, ids=WIDTH_IDS)
def test_query_widths_other_streams(geoms, dM, nq, k):
    geoms(*dM).check_preassigned(1, NLIST, k, nq)


# ---------------------------------------------------------------- c. list lengths
@pytest.fixture(scope="module", params=[32, 16, 8], ids=["dsub2", "dsub4", "dsub8"])
def exact_lengths(amd, orc, gpu, request):
    M = request.param
    cent, xb, xq = pf.exact_lengths_set(orc.float_rand, pf.RR_D)
    idx = pf.filled_ivfpq(amd, cent, M, xb, xb)
    assert [idx.get_list_size(l) for l in range(NLIST)] == pf.LENGTHS
    idx.nprobe = NLIST
    ref = orc.IVFOracle.from_index(idx)
    return idx, xq, ref.search(xq, 10, NLIST, nslices=1)


@pytest.mark.parametrize("nq", [33, 129])
def test_exact_list_lengths(amd, exact_lengths, nq):
    idx, xq, (Dr, Ir, _, _) = exact_lengths
    x = np.ascontiguousarray(xq[:nq])
    (D, I), names = pf.ran_stages(amd, idx, lambda: idx.search(x, 10))
    pf.assert_filter_ran(names)
    assert_same_results(D, I, Dr[:nq], Ir[:nq])


# ---------------------------------------------------------------- d. task walk
WALK_NLIST, WALK_NB, WALK_NQ, WALK_NPROBE = 8192, 20480, 512, 16


@pytest.fixture(scope="module")
def task_walk(amd, orc, gpu):
    """M8 d64 over 8192 random centroids, 2 or 3 rows beside each: 512 x 16
    probes fall on about 4000 lists, one work item each (4096 lists give
    about 2800) — more than the 12 waves x CUs x 2 tasks of two full rounds
    on 256 CUs, which take 3079 items."""
    d = 64
    cent = rand(orc, WALK_NLIST, d, 5601)
    xb = np.ascontiguousarray(cent[np.arange(WALK_NB) % WALK_NLIST] +
                              np.float32(0.05) * rand(orc, WALK_NB, d, 5602))
    xq = rand(orc, WALK_NQ, d, 5603)
    idx = pf.filled_ivfpq(amd, cent, 8, xb, xb, ids=np.arange(WALK_NB, dtype=np.int64))
    idx.nprobe = WALK_NPROBE
    _, Iq = idx.quantizer.search(xq, WALK_NPROBE)
    sizes = np.array([idx.get_list_size(l) for l in range(WALK_NLIST)])
    per_list = np.bincount(Iq.ravel(), minlength=WALK_NLIST)
    # an empty list has no work item (ivf_bucket counts only rows' lists)
    items = int(((per_list + 63) // 64)[sizes > 0].sum())
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nstatic = 12 * cus
    print(f"task walk: CUs={cus} items={items} tasks={2 * items} round={nstatic} "
          f"rounds={-(-2 * items // nstatic)}")
    assert 2 * items > 2 * nstatic + 12, (items, cus)
    ref = orc.IVFOracle.from_index(idx)
    return idx, xq, ref.search(xq, 10, WALK_NPROBE, nslices=1)


@pytest.mark.parametrize("switch", [None, ("FAISS_AMD_PQ_SCHED", "stride"),
                                    ("FAISS_AMD_PQ_SCHED", "snake"), ("FAISS_AMD_PQ_WPB", "4")],
                         ids=["default", "stride", "snake", "wpb4"])
def test_task_walk_past_two_rounds(amd, task_walk, monkeypatch, switch):
    idx, xq, (Dr, Ir, _, _) = task_walk
    if switch:
        monkeypatch.setenv(*switch)
    (D, I), names = pf.ran_stages(amd, idx, lambda: idx.search(xq, 10))
    pf.assert_filter_ran(names)
    assert_same_results(D, I, Dr, Ir)


@pytest.mark.parametrize("k", [1, 10, 20])
@pytest.mark.parametrize("nq", [33, 129])
@pytest.mark.parametrize("dM", [(64, 16), (96, 48), (128, 16)], ids=["M16d64", "M48d96", "M16d128"])
def test_work_group_form(geoms, monkeypatch, dM, nq, k):
    # the 4-wave form keeps unfolded keys: the re-rank runs with fold = 0
    monkeypatch.setenv("FAISS_AMD_PQ_FILTER", "wg")
    geoms(*dM).check_preassigned(1, NLIST, k, nq)


# ---------------------------------------------------------------- e. re-rank rare paths
DSUB_M = [32, 16, 8]
DSUB_IDS = ["dsub2", "dsub4", "dsub8"]


def stats_search(amd, orc, idx, xq, k, nprobe, monkeypatch, capfd):
    """search with FAISS_AMD_IVF_STATS=1 against the oracle: (D, counters)."""
    idx.nprobe = nprobe
    Dr, Ir, _, _ = orc.IVFOracle.from_index(idx).search(xq, k, nprobe, nslices=1)
    monkeypatch.setenv("FAISS_AMD_IVF_STATS", "1")
    capfd.readouterr()
    (D, I), names = pf.ran_stages(amd, idx, lambda: idx.search(xq, k))
    st = pf.scan_stats(capfd.readouterr().err)
    pf.assert_filter_ran(names)
    assert_same_results(D, I, Dr, Ir)
    return D, st


@pytest.fixture(scope="module", params=DSUB_M, ids=DSUB_IDS)
def tied(amd, orc, gpu, request):
    train, xb, xq = pf.ties_set(orc.float_rand)
    idx = amd.index_factory(pf.RR_D, f"IVF16,PQ{request.param}x8")
    idx.train(train)
    idx.add_with_ids(xb, pf.permuted_ids(xb.shape[0]))
    return idx, xq


@pytest.mark.parametrize("k", [10, 16])
def test_kth_key_tied_for_every_query(amd, orc, tied, monkeypatch, capfd, k):
    # 25 copies (one code) and k < 25: the k-th and the (k + 1)-th distance are
    # equal, and which ids survive is the reference's arrival order
    idx, xq = tied
    D, st = stats_search(amd, orc, idx, xq, k, 4, monkeypatch, capfd)
    ntied = int((D[:, 0] == D[:, k - 1]).sum())
    print(f"ties M{idx.pq_info()['M']} k={k}: tied queries {ntied}/{xq.shape[0]} {st}")
    assert ntied >= xq.shape[0] // 2


@pytest.mark.parametrize("M", DSUB_M, ids=DSUB_IDS)
def test_list_the_kept_keys_cannot_certify(amd, orc, gpu, monkeypatch, capfd, M):
    cent, train, xb, xq = pf.uncertifiable_set(orc.float_rand)
    idx = pf.filled_ivfpq(amd, cent, M, train, xb)
    D, st = stats_search(amd, orc, idx, xq, 10, 8, monkeypatch, capfd)
    print(f"failing streams M{M}: {st}")
    assert st["failing"] > 0.0, st


@pytest.mark.parametrize("M", DSUB_M, ids=DSUB_IDS)
def test_candidate_overflow_and_general_resolve(amd, orc, gpu, monkeypatch, capfd, M):
    # 700 copies of one vector: every stream of the list fails at its kept
    # keys' own value, 700 candidates > RR_CAP = 512
    cent, train, xb, xq = pf.uncertifiable_set(orc.float_rand, big_rows=700, copies=True)
    idx = pf.filled_ivfpq(amd, cent, M, train, xb)
    assert idx.get_list_size(15) == 700
    D, st = stats_search(amd, orc, idx, np.ascontiguousarray(xq[:32]), 10, 8, monkeypatch, capfd)
    print(f"overflow M{M}: {st}")
    assert st["overflow"] > 0 and st["general"] > 0, st
    assert (D[:, 0] == D[:, 9]).all()


@pytest.mark.parametrize("M", DSUB_M, ids=DSUB_IDS)
def test_candidate_count_edges(amd, orc, gpu, monkeypatch, capfd, M):
    cent, train, xb, xq = pf.candidate_count_set(orc.float_rand)
    idx = pf.filled_ivfpq(amd, cent, M, train, xb)
    n = len(pf.COUNT_SIZES)
    assert [idx.get_list_size(i) for i in range(n)] == pf.COUNT_SIZES
    D, st = stats_search(amd, orc, idx, xq, 10, 4, monkeypatch, capfd)
    print(f"candidate counts M{M}: {st}")
    assert (D[:, 0] == D[:, 9]).all()


# ---------------------------------------------------------------- f. max_codes
@pytest.fixture(scope="module")
def capped(amd, orc, gpu):
    """IVF64,PQ16x8, d = 64; 100 of the 300 queries are base rows from the
    last quarter of their lists: under a cap their true neighbours lie in
    the part of the list that is cut off."""
    d, nb, nq = 64, 12000, 300
    xb = rand(orc, nb, d, 5701)
    xq = rand(orc, nq, d, 5702).copy()
    idx = amd.index_factory(d, "IVF64,PQ16x8")
    idx.train(xb)
    idx.add(xb)
    off, _, ids = idx.invlists_arrays()
    rng = np.random.RandomState(11)
    for i in range(100):
        l = i % 64
        ln = int(off[l + 1] - off[l])
        assert ln >= 8
        xq[i] = xb[ids[off[l] + rng.randint(ln - ln // 4, ln)]]
    return idx, np.ascontiguousarray(xq), orc.IVFOracle.from_index(idx)


@pytest.mark.parametrize("max_codes", [1, 150, 700, 2000])
def test_max_codes_cuts_the_nearest_rows(amd, capped, max_codes):
    idx, xq, ref = capped
    k, nprobe = 10, 8
    Dq, Iq = idx.quantizer.search(xq, nprobe)
    idx.nprobe = nprobe
    idx.max_codes = max_codes
    st = amd.cvar.indexIVF_stats
    st.reset()
    try:
        (D, I), names = pf.ran_stages(amd, idx, lambda: idx.search_preassigned(xq, k, Iq, Dq))
    finally:
        idx.max_codes = 0
    ndis = st.ndis
    pf.assert_filter_ran(names)
    Dr, Ir, ndr = ref.search_preassigned(xq, k, Iq, Dq, max_codes=max_codes, return_ndis=True)
    assert_same_results(D, I, Dr, Ir)
    assert ndis == ndr <= xq.shape[0] * max_codes
    if max_codes <= 150:
        # the planted queries' own rows are cut off: an exact match (distance
        # of the row's own code) would otherwise lead their results
        D0, I0 = ref.search_preassigned(xq[:100], k, Iq[:100], Dq[:100])
        assert (I0[:, 0] != Ir[:100, 0]).sum() >= 50
