"""The re-ranks' rare paths against the oracle, bit for bit: a k-th key that is
tied for every query (IVF-Flat re-rank, and the coarse re-rank, whose small
select resolves the tie on the keys it holds: exact_select.h
exact_topk_tied_small), a list the filter's kept keys cannot certify (failing
streams), and candidate counts on both sides of every batch boundary of the
small selects (64 | 65, 128, 256 | 257).  L2 and inner product for each.
"""
import re

import numpy as np
import pytest

from conftest import assert_same_results, rand

pytestmark = pytest.mark.gpu

METRICS = ["l2", "ip"]


def ivf_on(amd, cent, metric):
    """IVF-Flat over the given centroids (a filled quantizer needs no training)."""
    d = cent.shape[1]
    if metric == "l2":
        quant, mt = amd.IndexFlatL2(d), amd.METRIC_L2
    else:
        quant, mt = amd.IndexFlatIP(d), amd.METRIC_INNER_PRODUCT
    quant.add(np.ascontiguousarray(cent))
    idx = amd.IndexIVFFlat(quant, d, cent.shape[0], mt)
    idx.train(cent)
    return idx


def same_as_oracle(orc, idx, xq, k, nprobe):
    idx.nprobe = nprobe
    D, I = idx.search(xq, k)
    Dr, Ir, _, _ = orc.IVFOracle.from_index(idx).search(xq, k, nprobe, nslices=1)
    assert_same_results(D, I, Dr, Ir)
    return D, I


# ---------------------------------------------------------------- ties
@pytest.fixture(scope="module")
def x25(amd, orc, gpu):
    """IVF16,Flat, d = 16, 80 vectors 25 times each (2000 rows, shuffled), per metric."""
    d, nu, copies = 16, 80, 25
    base = rand(orc, nu, d, 5101)
    perm = np.random.default_rng(3).permutation(nu * copies)
    xb = np.ascontiguousarray(np.repeat(base, copies, axis=0)[perm])
    xq = np.ascontiguousarray(np.concatenate([base[:32], rand(orc, 32, d, 5102)]))
    out = {}
    for metric in METRICS:
        mt = amd.METRIC_L2 if metric == "l2" else amd.METRIC_INNER_PRODUCT
        idx = amd.index_factory(d, "IVF16,Flat", mt)
        idx.train(base)
        idx.add(xb)
        out[metric] = idx
    return out, xq


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [10, 16])
def test_kth_key_tied_for_every_query(orc, x25, metric, k):
    # 25 copies and k < 25: the k-th and the (k + 1)-th key are equal in every
    # query whose nearest vector's copies are all probed
    idx, xq = x25
    D, I = same_as_oracle(orc, idx[metric], xq, k, 4)
    assert (D[:, 0] == D[:, k - 1]).sum() >= xq.shape[0] // 2


def tripled(orc, nlist, d, seed):
    """nlist centroids: nlist // 3 random ones three times each, the rest at
    the origin (last in either metric for data in [0, 1)^d).  In distance
    order the groups end at ranks 3, 6, ..., so rank 32 | 33 falls inside a
    group and the 32nd coarse key is tied for every query (pairs would end a
    group exactly at 32)."""
    c = np.zeros((nlist, d), np.float32)
    c[:nlist // 3 * 3] = np.repeat(rand(orc, nlist // 3, d, seed), 3, axis=0)
    return np.ascontiguousarray(c[np.random.default_rng(5).permutation(nlist)])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nlist", [64, 256])
def test_coarse_kth_key_tied_for_every_query(amd, orc, gpu, monkeypatch, capfd, metric, nlist):
    # d = 128, nprobe = 32 over duplicated centroids.  64 centroids are one
    # split, which the f32 tile answers; 256 have a filter plan, so there the
    # coarse re-rank's relayed queries meet the tie (and must all be relayed)
    d, nprobe, k = 128, 32, 10
    cent = tripled(orc, nlist, d, 5103)
    idx = ivf_on(amd, cent, metric)
    idx.add(rand(orc, 4000, d, 5104))
    xq = rand(orc, 64, d, 5105)
    m = 1 if metric == "l2" else 0
    Dr, Ir = orc.knn(xq, cent, nprobe, metric=m, blas_form=True)
    assert (Dr[:, nprobe - 1] == Dr[:, nprobe - 2]).all()  # a group of three ends past rank 32
    monkeypatch.setenv("FAISS_AMD_IVF_STATS", "1")
    capfd.readouterr()
    Dq, Iq = idx.quantizer.search(xq, nprobe)
    err = capfd.readouterr().err
    assert_same_results(Dq, Iq, Dr, Ir)
    if nlist == 256:
        st = re.findall(r"coarse bf3: nq=(\d+) k=(\d+) .*relayed=(\d+)", err)
        assert st, err[-400:]
        assert [int(v) for v in st[-1]] == [xq.shape[0], nprobe, xq.shape[0]]
    monkeypatch.delenv("FAISS_AMD_IVF_STATS")
    same_as_oracle(orc, idx, xq, k, nprobe)


# ---------------------------------------------------------------- failing streams
@pytest.mark.parametrize("metric", METRICS)
def test_list_the_kept_keys_cannot_certify(amd, orc, gpu, monkeypatch, capfd, metric):
    # 15 lists of 20 rows and one of 600 rows within 1e-3 of its centroid:
    # each of its streams holds 150 rows whose keys the filter cannot tell
    # apart and keeps KT of them, so for the queries beside it the streams fail
    d, k, nprobe = 32, 10, 8
    cent = rand(orc, 16, d, 5106)
    rng = np.random.default_rng(9)
    small = np.repeat(cent[:15], 20, axis=0) + 0.02 * rng.standard_normal((300, d))
    big = cent[15] + 1e-3 * rng.standard_normal((600, d))
    xb = np.ascontiguousarray(np.concatenate([small, big]).astype(np.float32))
    xq = np.ascontiguousarray(np.concatenate(
        [cent[15] + 1e-3 * rng.standard_normal((32, d)), rand(orc, 32, d, 5107)]).astype(np.float32))
    idx = ivf_on(amd, cent, metric)
    idx.add(xb)
    monkeypatch.setenv("FAISS_AMD_IVF_STATS", "1")
    capfd.readouterr()
    same_as_oracle(orc, idx, xq, k, nprobe)
    err = capfd.readouterr().err
    m = re.findall(r"ivf mfma scan: .*failing probes/q=([0-9.]+)", err)
    assert m, err[-400:]
    print(f"failing probes/q={m[-1]}")
    assert float(m[-1]) > 0.0, err[-400:]


# ---------------------------------------------------------------- candidate counts
SIZES = [64, 65, 128, 256, 257]


@pytest.mark.parametrize("metric", METRICS)
def test_candidate_count_edges(amd, orc, gpu, monkeypatch, tmp_path, metric):
    # list i holds SIZES[i] copies of its own centroid; the centroids are far
    # apart (orthogonal directions, norm 4).  A query beside centroid i has U
    # at that list's distance: every stream of the list keeps all its rows or
    # drops some at the kept ones' own key and fails, and no other list comes
    # under U, so the query has exactly SIZES[i] candidates (the re-rank
    # trace's word 2), all at one distance
    d, k, nprobe = 16, 10, 4
    cent = np.zeros((8, d), np.float32)
    cent[np.arange(8), np.arange(8)] = 4.0
    cent += rand(orc, 8, d, 5108) * np.float32(0.01)
    xb = np.ascontiguousarray(np.concatenate(
        [np.repeat(cent[i:i + 1], n, axis=0) for i, n in enumerate(SIZES)] +
        [np.repeat(cent[5:8], 12, axis=0)]))
    rng = np.random.default_rng(13)
    xq = np.ascontiguousarray(
        (np.repeat(cent[:5], 4, axis=0) + 0.01 * rng.standard_normal((20, d))).astype(np.float32))
    idx = ivf_on(amd, cent, metric)
    idx.add(xb)
    assert [idx.get_list_size(i) for i in range(5)] == SIZES
    trace = tmp_path / "rtrace.bin"
    monkeypatch.setenv("FAISS_AMD_RERANK_TRACE", str(trace))
    D, I = same_as_oracle(orc, idx, xq, k, nprobe)
    rec = np.fromfile(trace, dtype=np.uint64).reshape(-1, 8)
    ns = (rec[:, 2] & np.uint64(0xffffffff)).astype(np.int64)
    print(f"{metric}: candidates per query {ns}")
    assert ns.shape[0] == xq.shape[0]
    assert (ns == np.repeat(SIZES, 4)).all()
    assert (D[:, 0] == D[:, k - 1]).all()
