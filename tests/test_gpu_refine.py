"""IndexRefineFlat search on the GPU against reference runs.

Every expected array in tests/golden/ref_refine.npz was produced by the
reference library (scripts/make_golden_refine.py) from the index files in
tests/golden/ref_refine/, whose nprobe and k_factor fields are the case's.  Ids
and distances must be equal bit for bit: the re-rank kernel
(csrc/kernels_refine.hip) evaluates the reference's fp32 order (csrc/ref_arith.h)
and the exact select (csrc/kernels_exact.hip) reproduces reorder_2_heaps,
including the planted exact-distance ties whose survivor depends on the base
result's order and the padded rows of pq_l2_d64_np1."""
import os

import numpy as np
import pytest

from conftest import assert_same_results, device_search, rand

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = ["pq_l2_d64", "pq_l2_d64_kf25", "pq_l2_d64_np1", "flat_ip_d40", "flat_ip_d44",
        "sq8_l2_d72", "pq_l2_d96_k1", "sq8_ip_d40"]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_refine.npz"))


@pytest.fixture(scope="module")
def indexes(amd, gpu):
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = amd.read_index(os.path.join(HERE, "golden", "ref_refine", tag + ".faiss"))
        return cache[tag]
    return get


def expected(fx, tag, k):
    return fx[f"{tag}_{k}_D"], fx[f"{tag}_{k}_I"].astype(np.int64)


@pytest.mark.parametrize("tag", TAGS)
def test_search_equals_reference(indexes, fx, tag):
    idx = indexes(tag)
    for k in fx[f"{tag}_ks"]:
        D, I = idx.search(fx[f"{tag}_xq"], int(k))
        assert_same_results(D, I, *expected(fx, tag, int(k)))
    if tag == "pq_l2_d64_np1":  # the pads as the reference writes them
        D, I = idx.search(fx[f"{tag}_xq"], 100)
        assert (I < 0).any() and (D[I < 0] == np.finfo(np.float32).max).all()


@pytest.mark.parametrize("tag", ["pq_l2_d64", "flat_ip_d44", "pq_l2_d96_k1"])
def test_device_path(indexes, fx, tag):
    idx = indexes(tag)
    xq = fx[f"{tag}_xq"]
    D, I = idx.search(xq, 10)
    Dd, Id = device_search(idx, xq, 10)
    assert_same_results(Dd, Id, D, I)
    assert_same_results(Dd, Id, *expected(fx, tag, 10))


def test_params(amd, indexes, fx):
    xq = fx["pq_l2_d64_xq"]
    ivf4 = amd.SearchParametersIVF(nprobe=4)
    params = amd.IndexRefineSearchParameters(k_factor=4, base_index_params=ivf4)
    # files whose own fields are (nprobe 1, k_factor 4) and (nprobe 4, k_factor 2.5)
    for tag in ("pq_l2_d64_np1", "pq_l2_d64_kf25"):
        for k in (1, 10, 100):
            D, I = indexes(tag).search(xq, k, params=params)
            assert_same_results(D, I, *expected(fx, "pq_l2_d64", k))
    kf25 = amd.IndexRefineSearchParameters(k_factor=2.5)  # base parameters: the index's own
    D, I = indexes("pq_l2_d64").search(xq, 3, params=kf25)
    assert_same_results(D, I, *expected(fx, "pq_l2_d64_kf25", 3))
    idx = indexes("pq_l2_d64")
    with pytest.raises(amd.FaissError, match="incorrect type"):
        idx.search(xq, 10, params=ivf4)
    with pytest.raises(amd.FaissError, match="k_base >= k"):
        idx.search(xq, 10, params=amd.IndexRefineSearchParameters(k_factor=0.5))
    with pytest.raises(amd.FaissError, match="2048"):  # k_base = 2400: the base index's limit
        idx.search(xq, 600)
    D, I = idx.search(xq, 10)  # the index still serves after the errors
    assert_same_results(D, I, *expected(fx, "pq_l2_d64", 10))


def test_stage_timer(amd, indexes, fx):
    idx = indexes("pq_l2_d64")
    amd.set_kernel_timing(True)
    try:
        idx.reset_kernel_times()
        idx.search(fx["pq_l2_d64_xq"], 10)
        times = idx.kernel_times()
    finally:
        amd.set_kernel_timing(False)
        idx.reset_kernel_times()
    refine = [ms for name, ms, _ in times if name == "refine"]
    assert len(refine) == 1 and refine[0] > 0
    assert len(times) > 1  # the base index's stages are reported with it


def test_built_here(amd, gpu, orc, tmp_path):
    d, nb = 32, 3000
    xb, xq = rand(orc, nb, d, 901), rand(orc, 40, d, 902)
    idx = amd.index_factory(d, "IVF16,PQ8,RFlat")
    assert not idx.is_trained
    idx.train(xb)
    assert idx.is_trained
    idx.add(xb[:1700])
    idx.add(xb[1700:])
    assert (idx.ntotal, idx.base_index.ntotal, idx.refine_index.ntotal) == (nb, nb, nb)
    idx.k_factor = 5
    idx.base_index.nprobe = 6
    D, I = idx.search(xq, 10)
    f = tmp_path / "rf.faiss"
    amd.write_index(idx, f)
    back = amd.read_index(f)
    assert type(back) is amd.IndexRefineFlat and back.k_factor == 5 and back.base_index.nprobe == 6
    assert (back.ntotal, back.base_index.ntotal, back.refine_index.ntotal) == (nb, nb, nb)
    assert_same_results(*back.search(xq, 10), D, I)
    # the refined distances are exact, and no worse a choice than the base's own top 10
    for i in (0, 17, 39):
        for j in range(10):
            assert D[i, j] == np.float32(orc.fvec_L2sqr(xq[i], xb[I[i, j]]))
    _, Ib = idx.base_index.search(xq, 10)
    exact_of_base = np.array([[orc.fvec_L2sqr(xq[i], xb[j]) for j in Ib[i]] for i in range(40)])
    assert (D[:, -1] <= exact_of_base.max(axis=1)).all()
    idx.reset()
    assert (idx.ntotal, idx.base_index.ntotal, idx.refine_index.ntotal) == (0, 0, 0)
    # a flat base on duplicate-free data: the wrapper returns IndexFlat.search's
    # result (16 queries: below 20 the flat index computes fvec_L2sqr directly,
    # so its distances are the exact ones bit for bit)
    flat = amd.index_factory(d, "Flat,RFlat")
    flat.add(xb)
    flat.k_factor = 2
    plain = amd.IndexFlatL2(d)
    plain.add(xb)
    assert_same_results(*flat.search(xq[:16], 10), *plain.search(xq[:16], 10))


def test_range_search(amd, indexes, fx, orc):
    for tag, l2 in (("pq_l2_d64", True), ("flat_ip_d40", False)):
        idx = indexes(tag)
        xq = fx[f"{tag}_xq"]
        xb = idx.refine_index.xb
        Db, _ = idx.base_index.search(xq, 10)
        radius = float(np.median(Db[:, 5]))
        lims_b, D_b, I_b = idx.base_index.range_search(xq, radius)
        lims, D, I = idx.range_search(xq, radius)
        assert lims[-1] > 32 and np.array_equal(lims, lims_b) and np.array_equal(I, I_b)
        fn = orc.fvec_L2sqr if l2 else orc.fvec_inner_product
        want = np.array([fn(xq[i], xb[I[j]]) for i in range(32)
                         for j in range(lims[i], lims[i + 1])], np.float32)
        assert np.array_equal(D, want)
        if l2:
            # PQ distances scatter around the exact ones: some hits are beyond
            # the radius once refined, and stay (no second filter)
            assert (D >= radius).any() and not np.array_equal(D, D_b)
    ivf2 = amd.SearchParametersIVF(nprobe=2)
    idx, xq = indexes("pq_l2_d64"), fx["pq_l2_d64_xq"]
    lims2, _, I2 = idx.range_search(xq, 6.0, params=amd.IndexRefineSearchParameters(1, ivf2))
    lims2b, _, I2b = idx.base_index.range_search(xq, 6.0, params=ivf2)
    assert np.array_equal(lims2, lims2b) and np.array_equal(I2, I2b)


def reorder_2_heaps(k, dis, ids, l2):
    """faiss/IndexRefine.cpp:65-87 restated on a plain list: the heap's top is
    its largest (distance, id) (CMax, L2) / smallest (CMin, IP); the first k
    candidates are pushed unconditionally, a later one replaces the top when
    the top's distance is strictly worse; the result pops in order, drops
    label -1 and pads with (neutral, -1)."""
    key = (lambda t: t) if l2 else (lambda t: (-t[0], -t[1]))
    heap = [(np.float32(dis[i]), int(ids[i])) for i in range(k)]
    for i in range(k, len(dis)):
        top = max(heap, key=key)
        if (top[0] > dis[i]) if l2 else (top[0] < dis[i]):
            heap.remove(top)
            heap.append((np.float32(dis[i]), int(ids[i])))
    out = sorted((t for t in heap if t[1] != -1), key=key)
    neutral = np.finfo(np.float32).max * (1 if l2 else -1)
    out += [(neutral, -1)] * (k - len(out))
    return np.array([t[0] for t in out], np.float32), np.array([t[1] for t in out], np.int64)


def composed(orc, xq, xb, Ib, k, l2):
    """The reference's steps 2 and 3 on the host: oracle distances of the base
    result's labels, then reorder_2_heaps."""
    fn = orc.fvec_L2sqr if l2 else orc.fvec_inner_product
    bad = np.float32(np.inf if l2 else -np.inf)
    out = []
    for i in range(len(xq)):
        dis = [np.float32(fn(xq[i], xb[j])) if j >= 0 else bad for j in Ib[i]]
        out.append(reorder_2_heaps(k, dis, Ib[i], l2))
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def test_k_beyond_the_lds_select(amd, gpu, orc):
    """k > 2048: the select's arrays live in global scratch.  Only a flat base
    index serves such a k_base (the IVF indexes stop at 2048)."""
    d, nb, nq, k = 16, 2600, 2, 2100
    xb, xq = rand(orc, nb, d, 931), rand(orc, nq, d, 932)
    idx = amd.index_factory(d, "Flat,RFlat")
    idx.add(xb)
    idx.k_factor = 1.2
    k_base = int(k * np.float32(1.2))
    assert k_base == 2520
    _, Ib = idx.base_index.search(xq, k_base)
    D, I = idx.search(xq, k)
    assert_same_results(D, I, *composed(orc, xq, xb, Ib, k, True))


@pytest.mark.parametrize("d, desc, l2", [(4, "IVF64,PQ2,RFlat", True),
                                         (7, "IVF64,Flat,RFlat", False),
                                         (264, "IVF64,PQ33,RFlat", True),
                                         (13, "IVF64,Flat,RFlat", True),
                                         (100, "IVF64,PQ25,RFlat", False)])
def test_d_fallback(amd, gpu, orc, d, desc, l2):
    """Dimensions outside the four-lanes-per-row form (d < 8, d > 128): one
    lane per row; and two shapes of that form no fixture has: d = 13 (a scalar
    tail after the 4-term epilogue, XM = 8) and inner product at d = 100
    (XM = 16 with an epilogue).  Expected result composed on the host from the
    base index's own result, oracle distances and reorder_2_heaps."""
    nb, nq, k, kf = 1200, 24, 5, 6.5
    xb, xq = rand(orc, nb, d, 911 + d), rand(orc, nq, d, 912 + d)
    idx = amd.index_factory(d, desc, amd.METRIC_L2 if l2 else amd.METRIC_INNER_PRODUCT)
    idx.train(xb)
    idx.add(xb)
    idx.k_factor = kf
    idx.base_index.nprobe = 1
    k_base = int(k * np.float32(kf))
    assert k_base == 32
    _, Ib = idx.base_index.search(xq, k_base)
    if l2:  # lists of ~19 rows: most base rows end in -1 (inner-product lists are uneven)
        assert (Ib[:, k:] < 0).any()
    D, I = idx.search(xq, k)
    assert_same_results(D, I, *composed(orc, xq, xb, Ib, k, l2))
