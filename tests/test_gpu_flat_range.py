"""GPU: IndexFlat::range_search (faiss/IndexFlat.cpp:71-90 ->
faiss/utils/distances.cpp:940-966, RangeSearchBlockResultHandler).

lims, labels and distances must equal the reference's bit for bit: the
reference-run fixtures (tests/golden/ref_flat_range.npz) where they exist, else
the host restatement that tests/test_flat_range_fixtures.py pins against them
(tests/flat_range_ref.py).  A selector or fewer than 20 queries take the direct
form (fvec_L2sqr / fvec_inner_product per pair over is_member), anything else
the BLAS form; hits of a query come in ascending row order; the comparison is
strict."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flat_range_ref as fr
from conftest import rand
from flat_range_ref import CASES, load_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(fr.GOLD)


def flat(amd, xb, metric_l2):
    idx = amd.index_factory(xb.shape[1], "Flat",
                            amd.METRIC_L2 if metric_l2 else amd.METRIC_INNER_PRODUCT)
    if xb.shape[0]:
        idx.add(xb)
    return idx


def radius_at(full, metric_l2, frac):
    """The radius that admits about `frac` of the evaluated pairs."""
    v = np.sort(full[np.isfinite(full)])
    return float(v[int(frac * v.size)] if metric_l2 else v[v.size - 1 - int(frac * v.size)])


# ---- 1. the reference's own results
@pytest.mark.parametrize("tag", CASES)
def test_fixture_case_bit_exact(amd, orc, gpu, gold, tag):
    xq, xb, ml2, radius, want = load_case(gold, orc, tag)
    got = flat(amd, xb, ml2).range_search(xq, radius)
    fr.check_equal(got, want)


# ---- 2. shapes the fixtures do not cover, against the restatement
# nq = 20: exactly at the BLAS threshold; 130: crosses a 128-query tile;
# ntotal = 129 / 4100: cross the 128-row tile and the 1024 / 4096 row blocks;
# d = 4 / 33 / 264: one k-step short of a chunk, padded rows, many chunks
SHAPES = [(20, 129, 4), (130, 129, 33), (130, 129, 264), (20, 4100, 264), (130, 4100, 33),
          (19, 4100, 33), (7, 129, 264)]


@pytest.mark.parametrize("metric_l2", [True, False])
@pytest.mark.parametrize("nq,nb,d", SHAPES)
def test_shapes_equal_restatement(amd, orc, gpu, nq, nb, d, metric_l2):
    off = 0.0 if metric_l2 else 0.5
    xb = rand(orc, nb, d, 4100 + d) - np.float32(off)
    xq = rand(orc, nq, d, 4200 + d) - np.float32(off)
    full = fr.distance_matrix(orc, xq, xb, metric_l2, nq >= 20, per_pair=False)
    radius = radius_at(full, metric_l2, 0.02)
    want = fr.threshold(full, metric_l2, radius)
    assert 0 < want[0][-1] < 0.05 * nq * nb
    got = flat(amd, xb, metric_l2).range_search(xq, radius)
    fr.check_equal(got, want)


def test_query_chunks_join(amd, orc, gpu):
    """1M rows make 7813 count cells per query, so the 256 MiB count budget
    cuts 8706 queries into chunks of 8576 and 130: the call equals its two
    halves searched alone (each one chunk, both in the BLAS form), and sampled
    queries on both sides of the cut equal the restatement."""
    nb, d, cut, nq = 1000000, 4, 8576, 8576 + 130
    xb = rand(orc, nb, d, 4351)
    xq = rand(orc, nq, d, 4352)
    idx = flat(amd, xb, True)
    radius = 0.0005                      # about one hit per query
    lims, D, I = idx.range_search(xq, radius)
    la, Da, Ia = idx.range_search(xq[:cut], radius)
    lb, Db, Ib = idx.range_search(xq[cut:], radius)
    assert lims[-1] > nq // 2
    fr.check_equal((lims, D, I), (np.concatenate([la, lb[1:] + la[-1]]),
                                  np.concatenate([Da, Db]), np.concatenate([Ia, Ib])))
    sample = np.array([0, 1, cut - 1, cut, cut + 1, nq - 1])
    Dk, Ik = orc.knn(xq[sample], xb, 64, metric=1, blas_form=True)
    for s, q in enumerate(sample):
        hit = Dk[s] < np.float32(radius)
        assert not hit.all()
        order = np.argsort(Ik[s][hit])
        assert np.array_equal(I[lims[q]:lims[q + 1]], Ik[s][hit][order])
        assert np.array_equal(D[lims[q]:lims[q + 1]], Dk[s][hit][order])


# ---- 3. self-consistency with the exact k > 64 search path
@pytest.mark.parametrize("metric_l2", [True, False])
@pytest.mark.parametrize("nq", [37, 19])
def test_equals_full_search_filtered(amd, orc, gpu, nq, metric_l2):
    nb, d = 1500, 40
    xb = rand(orc, nb, d, 4301)
    xq = rand(orc, nq, d, 4302)
    idx = flat(amd, xb, metric_l2)
    D, I = idx.search(xq, nb)
    assert (I >= 0).all()
    full = np.empty((nq, nb), np.float32)
    np.put_along_axis(full, I, D, axis=1)
    radius = radius_at(full, metric_l2, 0.01)
    want = fr.threshold(full, metric_l2, radius)
    assert want[0][-1] > nq
    fr.check_equal(idx.range_search(xq, radius), want)


# ---- 4. selectors: the direct form over is_member, whatever the batch size
NB_SEL, D_SEL, NQ_SEL = 700, 40, 37


@pytest.fixture(scope="module")
def sel_data(amd, orc, gpu):
    xb = rand(orc, NB_SEL, D_SEL, 4401)
    xq = rand(orc, NQ_SEL, D_SEL, 4402)
    direct = fr.distance_matrix(orc, xq, xb, True, False)
    blas = fr.distance_matrix(orc, xq, xb, True, True)
    return xb, xq, direct, blas, flat(amd, xb, True)


def selectors(amd):
    rng = np.random.RandomState(44)
    batch = rng.choice(NB_SEL, 300, replace=False)
    arr = np.concatenate([rng.choice(NB_SEL, 200, replace=False), [5, 5, 130, 5]])
    bitmap = rng.randint(0, 256, (NB_SEL + 7) // 8).astype(np.uint8)
    rows = np.arange(NB_SEL)
    bit_member = ((bitmap[rows >> 3] >> (rows & 7)) & 1).astype(bool)
    return {
        "range": (lambda: amd.IDSelectorRange(100, 517), (rows >= 100) & (rows < 517)),
        "batch": (lambda: amd.IDSelectorBatch(batch), np.isin(rows, batch)),
        "array_repeated": (lambda: amd.IDSelectorArray(arr), np.isin(rows, arr)),
        "bitmap": (lambda: amd.IDSelectorBitmap(bitmap), bit_member),
        "not": (lambda: amd.IDSelectorNot(amd.IDSelectorBatch(batch)), ~np.isin(rows, batch)),
    }


@pytest.mark.parametrize("name", ["range", "batch", "array_repeated", "bitmap", "not"])
def test_selector_takes_direct_form(amd, orc, sel_data, name):
    xb, xq, direct, blas, idx = sel_data
    make, member = selectors(amd)[name]
    sel = make()
    assert all(sel.is_member(j) == bool(member[j]) for j in range(0, NB_SEL, 7))
    masked = np.where(member[None, :], direct, np.float32(np.nan))
    radius = radius_at(masked, True, 0.03)
    want = fr.threshold(masked, True, radius)
    # the two forms differ in at least one bit among these hits, so equality
    # below tells the direct form from the BLAS form
    qi = np.repeat(np.arange(NQ_SEL), np.diff(want[0]))
    assert (blas[qi, want[2]].view(np.uint32) != want[1].view(np.uint32)).any()
    # params of any SearchParameters subtype are accepted: only sel is read
    for params in (amd.SearchParametersIVF(sel=sel), amd.SearchParametersHNSW(sel=sel)):
        got = idx.range_search(xq, radius, params=params)
        fr.check_equal(got, want)
        # ascending rows: an id the array lists three times comes once
        for i in range(NQ_SEL):
            assert np.all(np.diff(got[2][got[0][i]:got[0][i + 1]]) > 0)


# ---- 5. edges
def test_no_queries(amd, orc, gpu):
    idx = flat(amd, rand(orc, 50, 8, 4501), True)
    lims, D, I = idx.range_search(np.zeros((0, 8), np.float32), 1.0)
    assert lims.tolist() == [0] and D.size == 0 and I.size == 0


@pytest.mark.parametrize("metric_l2", [True, False])
def test_empty_index(amd, orc, gpu, metric_l2):
    idx = flat(amd, np.zeros((0, 8), np.float32), metric_l2)
    lims, D, I = idx.range_search(rand(orc, 25, 8, 4502), 0.5 if metric_l2 else -0.5)
    assert lims.tolist() == [0] * 26 and D.size == 0 and I.size == 0


@pytest.mark.parametrize("nq", [37, 19])
def test_radius_edges(amd, orc, gpu, nq):
    nb, d = 300, 24
    xb = rand(orc, nb, d, 4503)
    xq = rand(orc, nq, d, 4504)
    xq[2] = xb[77]                      # distance exactly 0: not < 0
    l2, ip = flat(amd, xb, True), flat(amd, xb, False)
    for radius in (0.0, -1.0):          # L2: no hit
        lims, D, I = l2.range_search(xq, radius)
        assert lims.tolist() == [0] * (nq + 1) and D.size == 0
    every = np.tile(np.arange(nb), nq)
    for idx, ml2, radius in ((l2, True, 1e30), (ip, False, -1.0)):
        # every pair is a hit (inner products of non-negative data are > -1)
        got = idx.range_search(xq, radius)
        assert got[0][-1] == nq * nb and np.array_equal(got[2], every)
        fr.check_equal(got, fr.restate(orc, xq, xb, ml2, radius, per_pair=False))


@pytest.mark.parametrize("nq", [37, 19])
def test_non_finite(amd, orc, gpu, nq):
    """IP: a query with a +inf coordinate has +inf (a hit for a finite radius)
    or -inf / NaN (never one) with every row; a NaN row is never a hit, and an
    L2 distance of +inf never is."""
    nb, d = 300, 24
    xb = rand(orc, nb, d, 4505) - np.float32(0.5)
    xq = rand(orc, nq, d, 4506) - np.float32(0.5)
    xb[131, 3] = np.nan
    xq[4, 9] = np.inf
    for ml2, radius in ((False, 0.8), (True, 1.6), (True, np.inf)):
        want = fr.restate(orc, xq, xb, ml2, radius, per_pair=False)
        got = flat(amd, xb, ml2).range_search(xq, radius)
        fr.check_equal(got, want)
        assert 131 not in got[2]
        n4 = int(got[0][5] - got[0][4])
        if ml2:
            assert n4 == 0                       # +inf < radius never holds
        else:
            assert 0 < n4 < nb and np.all(np.isposinf(got[1][got[0][4]:got[0][5]]))
        if radius == np.inf:
            assert got[0][-1] == (nq - 1) * (nb - 1)   # every finite distance


# ---- 6. "Flat,RFlat"
@pytest.mark.parametrize("nq", [37, 12])
def test_refine_over_flat_base(amd, orc, gpu, nq):
    """IndexRefine::range_search (faiss/IndexRefine.cpp:169-206) takes the base
    index's hits and recomputes their distances from its flat storage, per pair
    (fvec_L2sqr).  The labels and lims are the flat base's in both forms; the
    distances are the base's own where the base took the direct form (nq < 20),
    and the direct form's distances of the base's BLAS-form hits otherwise."""
    nb, d = 900, 40
    xb = rand(orc, nb, d, 4601)
    xq = rand(orc, nq, d, 4602)
    idx = amd.index_factory(d, "Flat,RFlat")
    idx.add(xb)
    base = flat(amd, xb, True)
    full = fr.distance_matrix(orc, xq, xb, True, nq >= 20, per_pair=False)
    radius = radius_at(full, True, 0.02)
    want = base.range_search(xq, radius)
    fr.check_equal(want, fr.threshold(full, True, radius))
    got = idx.range_search(xq, radius)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    qi = np.repeat(np.arange(nq), np.diff(np.asarray(want[0], np.int64)))
    per_pair = np.array([orc.fvec_L2sqr(xq[i], xb[j]) for i, j in zip(qi, want[2])], np.float32)
    assert np.array_equal(got[1].view(np.uint32), per_pair.view(np.uint32))
    if nq < 20:
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


# ---- 7. the C API, read back by hand
def test_c_api_range_search(amd, orc, gpu):
    nb, d, nq = 500, 16, 30
    xb = rand(orc, nb, d, 4701)
    xq = rand(orc, nq, d, 4702)
    full = fr.distance_matrix(orc, xq, xb, True, True)
    radius = radius_at(full, True, 0.02)
    want = fr.threshold(full, True, radius)
    L = amd.lib()
    idx = flat(amd, xb, True)
    r = C.c_void_p()
    assert L.faiss_RangeSearchResult_new(C.byref(r), nq) == 0
    try:
        assert L.faiss_Index_range_search(idx.h, nq, xq.ctypes.data_as(C.c_void_p),
                                          C.c_float(radius), r) == 0
        assert L.faiss_RangeSearchResult_nq(r) == nq
        tot = L.faiss_RangeSearchResult_buffer_size(r)
        lp = C.POINTER(C.c_size_t)()
        L.faiss_RangeSearchResult_lims(r, C.byref(lp))
        lims = np.ctypeslib.as_array(lp, shape=(nq + 1,)).copy()
        assert tot == lims[-1] == want[0][-1] > 0
        ip, dp = C.POINTER(C.c_int64)(), C.POINTER(C.c_float)()
        L.faiss_RangeSearchResult_labels(r, C.byref(ip), C.byref(dp))
        got = (lims, np.ctypeslib.as_array(dp, shape=(tot,)).copy(),
               np.ctypeslib.as_array(ip, shape=(tot,)).copy())
    finally:
        L.faiss_RangeSearchResult_free(r)
    fr.check_equal(got, want)
    # a result sized for another batch is refused, as the IVF entry point does
    assert L.faiss_RangeSearchResult_new(C.byref(r), nq + 1) == 0
    try:
        assert L.faiss_Index_range_search(idx.h, nq, xq.ctypes.data_as(C.c_void_p),
                                          C.c_float(radius), r) != 0
    finally:
        L.faiss_RangeSearchResult_free(r)


def test_hnsw_range_search_stays_unimplemented(amd, orc, gpu):
    idx = amd.index_factory(8, "HNSW8")
    idx.add(rand(orc, 100, 8, 4703))
    with pytest.raises(amd.FaissError, match="range search not implemented"):
        idx.range_search(rand(orc, 3, 8, 4704), 1.0)


# ---- 8. the C++ drop-in: <faiss/IndexFlat.h>, faiss::IndexFlatL2::range_search
CPP = r"""
#include <faiss/IndexFlat.h>
#include <faiss/impl/AuxIndexStructures.h>
#include <cstdio>
#include <vector>
int main() {
    const int d = 8, nb = 300, nq = 25;   // multiples of 1/4: every form is exact
    std::vector<float> xb(nb * d), xq(nq * d);
    for (int i = 0; i < nb; i++)
        for (int j = 0; j < d; j++) xb[i * d + j] = ((i * 7 + j * 3) % 11) * 0.25f;
    for (int i = 0; i < nq; i++)
        for (int j = 0; j < d; j++) xq[i * d + j] = ((i * 5 + j * 2) % 11) * 0.25f;
    faiss::IndexFlatL2 index(d);
    index.add(nb, xb.data());
    faiss::RangeSearchResult res(nq);
    index.range_search(nq, xq.data(), 4.0f, &res);
    for (int i = 0; i < nq; i++) {
        std::printf("%d:", i);
        for (size_t j = res.lims[i]; j < res.lims[i + 1]; j++)
            std::printf(" %lld=%g", (long long)res.labels[j], (double)res.distances[j]);
        std::printf("\n");
    }
    return 0;
}
"""


def test_cpp_shim_range_search(amd, gpu, tmp_path):
    src, exe = tmp_path / "flat_range.cpp", tmp_path / "flat_range"
    src.write_text(CPP)
    libdir = os.path.join(ROOT, "hnsw-ivf_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o",
                    str(exe), f"-L{libdir}", "-lfaiss_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    i, j = np.arange(300)[:, None], np.arange(8)[None, :]
    xb = ((i * 7 + j * 3) % 11) * 0.25
    xq = ((i[:25] * 5 + j * 2) % 11) * 0.25
    dis = ((xq[:, None, :] - xb[None, :, :]) ** 2).sum(axis=2)
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 25
    nhit = 0
    for q, line in enumerate(lines):
        want = " ".join(f"{c}={dis[q, c]:g}" for c in np.nonzero(dis[q] < 4.0)[0])
        assert line == (f"{q}: {want}" if want else f"{q}:")
        nhit += int((dis[q] < 4.0).sum())
    assert nhit > 25
