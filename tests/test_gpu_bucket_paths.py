"""GPU parity of the IVF bucketing paths (kern::ivf_bucket) against the oracle,
bit for bit: the one-launch path (n * nprobe <= 16384 and nlist <= 8192: one
work group builds the histogram, scans it and fills), the two-launch path
(count, then a fill whose work groups scan the counts themselves and whose
last group clears them) and, past 8192 lists, the unchanged scan kernels.

Item numbering cannot change a result, but a wrong item offset, a wrong count
of queries in an item or a wrong descriptor does: the shapes put several items
in a list, a one-entry last item, an exact multiple of the item size, lists
that nobody probes, probes of empty lists and invalid probes, list counts that
are no multiple of four, and both sides of every dispatch threshold.
"""
import numpy as np
import pytest

from conftest import assert_same_results, rand

pytestmark = pytest.mark.gpu

ONE_MAX = 16384  # entries (n * nprobe) up to which one work group does the whole stage


def bucketed(amd, idx, fn):
    """fn() with the stage timers on; the bucket stage must have run."""
    amd.set_kernel_timing(True)
    try:
        idx.reset_kernel_times()
        out = fn()
        names = {nm for nm, _, _ in idx.kernel_times()}
    finally:
        amd.set_kernel_timing(False)
    assert "ivf_bucket" in names, names
    return out


def build_ivf(amd, orc, d, nb, nlist, desc="Flat", seed=1234, ntrain=None, nadd=None):
    xb = rand(orc, nb, d, seed)
    idx = amd.index_factory(d, f"IVF{nlist},{desc}")
    idx.train(xb[:ntrain] if ntrain else xb)
    idx.add(xb[:nadd] if nadd else xb)
    return idx, xb


def check_search(amd, orc, idx, ref, xq, k, nprobe):
    idx.nprobe = nprobe
    D, I = bucketed(amd, idx, lambda: idx.search(xq, k))
    Dr, Ir, _, _ = ref.search(xq, k, nprobe, nslices=1)
    assert_same_results(D, I, Dr, Ir)
    return I


def check_preassigned(amd, idx, ref, xq, k, nprobe, keys=None, cdis=None, must_bucket=True):
    idx.nprobe = nprobe
    if keys is None:
        cdis, keys = idx.quantizer.search(xq, nprobe)
    run = lambda: idx.search_preassigned(xq, k, keys, cdis)
    D, I = bucketed(amd, idx, run) if must_bucket else run()
    Dr, Ir = ref.search_preassigned(xq, k, keys, cdis)
    assert_same_results(D, I, Dr, Ir)
    return I


@pytest.fixture(scope="module")
def ivf64(amd, orc, gpu):
    idx, xb = build_ivf(amd, orc, 32, 4096, 64)
    return idx, orc.IVFOracle.from_index(idx)


# --- 1. the one-launch path and its upper edge (nprobe 8: 2048 queries are
# exactly 16384 entries, 2049 the first shape of the two-launch path)
@pytest.mark.parametrize("nq", [1, 100, 2048, 2049])
def test_one_launch_path_and_edge(amd, orc, ivf64, monkeypatch, nq):
    monkeypatch.setenv("FAISS_AMD_IVF_SCAN", "mfma")
    idx, ref = ivf64
    assert (nq * 8 <= ONE_MAX) == (nq <= 2048)
    check_search(amd, orc, idx, ref, rand(orc, nq, 32, 5000 + nq), 10, 8)


# --- 2. several items per list: every query probes every list, so a list's
# bucket holds nq entries (items of 128: full items, a one-entry last item,
# an exact multiple; 4097 * 4 = 16388 entries take the two-launch path)
@pytest.fixture(scope="module")
def ivf4(amd, orc, gpu):
    idx, xb = build_ivf(amd, orc, 16, 600, 4, seed=91)
    return idx, orc.IVFOracle.from_index(idx)


@pytest.mark.parametrize("nq", [127, 128, 129, 256, 257, 4097])
def test_items_per_list_flat(amd, orc, ivf4, monkeypatch, nq):
    monkeypatch.setenv("FAISS_AMD_IVF_SCAN", "mfma")
    idx, ref = ivf4
    assert (nq * 4 <= ONE_MAX) == (nq < 4097)
    check_search(amd, orc, idx, ref, rand(orc, nq, 16, 6000 + nq), 10, 4)


@pytest.fixture(scope="module", params=["PQ4x8", "PQ16x8"])
def ivf8pq(request, amd, orc, gpu):
    # PQ16x8 at d = 64 is served by the list-centric PQ filter (items of 64
    # queries); PQ4x8 at d = 16 by whichever scan serves that geometry
    desc = request.param
    d = 16 if desc == "PQ4x8" else 64
    idx, xb = build_ivf(amd, orc, d, 3000, 8, desc=desc, seed=92)
    return desc, d, idx, orc.IVFOracle.from_index(idx)


@pytest.mark.parametrize("nq", [63, 64, 65, 129])
def test_items_per_list_pq(amd, orc, ivf8pq, nq):
    desc, d, idx, ref = ivf8pq
    check_preassigned(amd, idx, ref, rand(orc, nq, d, 7000 + nq), 10, 8,
                      must_bucket=desc == "PQ16x8")


def test_items_per_list_pq_two_launch(amd, orc, ivf8pq):
    desc, d, idx, ref = ivf8pq
    nq = 2049  # 16392 entries, 33 items per list, the last of one entry
    check_preassigned(amd, idx, ref, rand(orc, nq, d, 7777), 10, 8,
                      must_bucket=desc == "PQ16x8")


# --- 3. list counts that are no multiple of four (the scans read four
# counts per load) on both paths, and the upper edge of both paths
@pytest.mark.parametrize("nq", [50, 3400])
def test_nlist_not_multiple_of_four(amd, orc, gpu, monkeypatch, nq):
    monkeypatch.setenv("FAISS_AMD_IVF_SCAN", "mfma")
    idx, xb = build_ivf(amd, orc, 16, 2000, 37, seed=93)
    assert (nq * 5 <= ONE_MAX) == (nq == 50)
    check_search(amd, orc, idx, orc.IVFOracle.from_index(idx), rand(orc, nq, 16, 94), 10, 5)


@pytest.fixture(scope="module", params=[8192, 8193])
def ivf_many(request, amd, orc, gpu):
    idx, xb = build_ivf(amd, orc, 16, 20000, request.param, seed=95)
    return request.param, idx, orc.IVFOracle.from_index(idx)


@pytest.mark.parametrize("nprobe", [16, 64])
def test_upper_edge_of_nlist(amd, orc, ivf_many, monkeypatch, nprobe):
    # 300 queries: nprobe 16 is 4800 entries (one launch at 8192 lists), nprobe
    # 64 is 19200 (two launches); 8193 lists keep the scan kernels either way
    monkeypatch.setenv("FAISS_AMD_IVF_SCAN", "mfma")
    nlist, idx, ref = ivf_many
    check_search(amd, orc, idx, ref, rand(orc, 300, 16, 96), 10, nprobe)


# --- 4. empty lists and invalid probes
@pytest.fixture(scope="module")
def ivf_sparse(amd, orc, gpu):
    # 64 lists trained, 40 vectors added: most probes hit empty lists
    idx, xb = build_ivf(amd, orc, 32, 2000, 64, seed=97, nadd=40)
    return idx, orc.IVFOracle.from_index(idx)


@pytest.mark.parametrize("nq", [200, 1100])
def test_mostly_empty_lists(amd, orc, ivf_sparse, monkeypatch, nq):
    monkeypatch.setenv("FAISS_AMD_IVF_SCAN", "mfma")
    idx, ref = ivf_sparse
    assert (nq * 16 <= ONE_MAX) == (nq == 200)
    # k = 32: a quarter of the lists cannot hold 32 of the 40 vectors here, so
    # every row ends in padding
    I = check_search(amd, orc, idx, ref, rand(orc, nq, 32, 98), 32, 16)
    assert (I[:, -1] == -1).all() and (I[:, 0] >= 0).any()


@pytest.mark.parametrize("nq,dups", [(300, False), (2100, False), (300, True), (2100, True)])
def test_preassigned_invalid_and_repeated_probes(amd, orc, ivf64, ivf_sparse, monkeypatch, nq, dups):
    monkeypatch.setenv("FAISS_AMD_IVF_SCAN", "mfma")
    rng = np.random.default_rng(nq + dups)
    for idx, ref in (ivf64, ivf_sparse):
        xq = rand(orc, nq, 32, 99)
        idx.nprobe = 8
        cdis, keys = idx.quantizer.search(xq, 8)
        keys = keys.copy()
        keys[rng.random(keys.shape) < 0.3] = -1
        keys[::7] = -1  # whole queries without a probe
        if dups:
            # a list named twice by a query (the scan then takes each probe
            # on its own, so the bucket stage need not run)
            keys[1::3, 5] = keys[1::3, 2]
            keys[2::5, 7] = keys[2::5, 0]
        check_preassigned(amd, idx, ref, xq, 10, 8, keys, cdis, must_bucket=not dups)


# --- 5. the counts and the ticket clean themselves: replayed graphs, a
# change of shape, a change of path; every call equals the oracle
@pytest.fixture(scope="module")
def replay_refs(orc, ivf64):
    idx, ref = ivf64
    out = {}
    for nq in (100, 300, 2500, 3000):
        xq = rand(orc, nq, 32, 8000 + nq)
        Dr, Ir, _, _ = ref.search(xq, 10, 8, nslices=1)
        out[nq] = (xq, Dr, Ir)
    return out


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("first,other", [(100, 300), (2500, 3000), (100, 2500), (2500, 100)])
def test_self_cleaning_under_replay(amd, ivf64, replay_refs, monkeypatch, graph, first, other):
    # 100 / 300 queries: one launch; 2500 / 3000: two.  Of four identical
    # calls the second is captured and the later ones replay the graph.
    monkeypatch.setenv("FAISS_AMD_IVF_SCAN", "mfma")
    monkeypatch.setenv("FAISS_AMD_GRAPH", graph)
    idx, _ = ivf64
    idx.nprobe = 8
    for nq in [first] * 4 + [other] * 4 + [first] * 4:
        xq, Dr, Ir = replay_refs[nq]
        D, I = idx.search(xq, 10)
        assert_same_results(D, I, Dr, Ir)


# --- 6. a selector and max_codes (they travel in the bucket struct) on the
# two-launch path
def test_selector_two_launch(amd, orc, gpu, monkeypatch):
    monkeypatch.setenv("FAISS_AMD_IVF_SCAN", "mfma")
    d, nb, nlist, nq = 32, 4096, 64, 2100
    xb = rand(orc, nb, d, 1234)
    q = amd.IndexFlatL2(d)
    full = amd.IndexIVFFlat(q, d, nlist)
    full.train(xb)
    full.add(xb)
    keep = np.nonzero(np.random.default_rng(5).random(nb) < 0.4)[0].astype(np.int64)
    sub = amd.IndexIVFFlat(q, d, nlist)
    sub.add_with_ids(xb[keep], keep)
    xq = rand(orc, nq, d, 101)
    full.nprobe = sub.nprobe = 8
    params = amd.SearchParametersIVF(nprobe=8, sel=amd.IDSelectorBatch(keep))
    D, I = bucketed(amd, full, lambda: full.search(xq, 10, params=params))
    Ds, Is = sub.search(xq, 10)
    assert_same_results(D, I, Ds, Is)
    Dr, Ir, _, _ = orc.IVFOracle.from_index(sub).search(xq, 10, 8, nslices=1)
    assert_same_results(D, I, Dr, Ir)


def test_max_codes_two_launch(amd, orc, ivf64, monkeypatch):
    monkeypatch.setenv("FAISS_AMD_IVF_SCAN", "mfma")
    idx, ref = ivf64
    xq = rand(orc, 2100, 32, 102)
    idx.nprobe = 8
    cdis, keys = idx.quantizer.search(xq, 8)
    idx.max_codes = 150
    try:
        D, I = bucketed(amd, idx, lambda: idx.search_preassigned(xq, 10, keys, cdis))
    finally:
        idx.max_codes = 0
    Dr, Ir = ref.search_preassigned(xq, 10, keys, cdis, max_codes=150)
    assert_same_results(D, I, Dr, Ir)
