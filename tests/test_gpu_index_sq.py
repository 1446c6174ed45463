"""IndexScalarQuantizer's full scan (csrc/kernels_sq_flat.hip) on the GPU.

Every comparison is exact: the reference's recorded results
(scripts/make_golden_index_sq.py) and the fp32 model of tests/sq_model.py
(decode, distances) under the reference heap (pq_nbits_model.heap_topk), rows
arriving in row order.  No tolerances."""
import functools
import os

import numpy as np
import pytest

import sq_model
from conftest import device_search

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_index_sq")
QT_8bit, QT_fp16 = 0, 4


def model_search(xq, codes, qtype, trained, l2, k, rows=None):
    """heap_topk over the model's distances to `rows` (all of them when None)."""
    d = xq.shape[1]
    rows = np.arange(len(codes)) if rows is None else np.asarray(rows)
    dist = sq_model.distances(xq, sq_model.decode(codes[rows], qtype, trained, d), l2)
    out = [sq_model.heap_topk(zip(dq.tolist(), rows.tolist()), k, l2) for dq in dist]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def same(D, I, Dm, Im):
    assert np.array_equal(I, Im), np.nonzero((I != Im).any(axis=1))[0][:5]
    assert np.array_equal(D, Dm, equal_nan=True)


@functools.lru_cache(maxsize=None)
def content(qtype, l2, d, n, nq, k):
    """Random ranges, codes and queries.  Of query 0's model ranking the 1st
    row is copied over the 2nd and the k-th over the two after it, so equal
    distances sit inside the result and straddle k."""
    rng = np.random.default_rng([77, qtype, l2, d, n, nq])
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    if qtype == QT_8bit:
        trained = np.concatenate([rng.standard_normal(d) - 1, rng.uniform(0.5, 3, d)]).astype(np.float32)
        codes = rng.integers(0, 256, (n, d), dtype=np.uint8)
    else:
        trained = np.zeros(0, np.float32)
        codes = np.ascontiguousarray(rng.standard_normal((n, d)).astype("<f2")).view(np.uint8)
    if n > 6:
        dist = sq_model.distances(xq[:1], sq_model.decode(codes, qtype, trained, d), l2)[0]
        order = np.argsort(dist if l2 else -dist, kind="stable")
        codes[order[1]] = codes[order[0]]
        if k < n:
            codes[order[k:k + 2]] = codes[order[k - 1]]
    return trained, codes, xq


def index_of(amd, qtype, l2, d, trained, codes):
    idx = amd.IndexScalarQuantizer(d, qtype, amd.METRIC_L2 if l2 else amd.METRIC_INNER_PRODUCT)
    idx.set_content(trained if qtype == QT_8bit else None, codes)
    return idx


@pytest.mark.parametrize("tag", ["sq8_l2_d40", "sq8_ip_d72", "sqfp16_l2_d24"])
def test_reference_fixtures(amd, gpu, tag):
    idx = amd.read_index(os.path.join(GOLDEN, tag + ".faiss"))
    f = np.load(os.path.join(GOLDEN, tag + ".npz"))
    same(*idx.search(f["xq"], 10), f["D"], f["I"])
    same(*device_search(idx, f["xq"], 10), f["D"], f["I"])


# d, ntotal, nq, k: the smallest of each; a slice plus a remainder and one row
# past a tile; a row pitch that is no multiple of 16 bytes and one query past a
# tile; many row tiles and k above 32; k > ntotal (pads)
SHAPES = [(8, 1, 1, 1), (40, 65, 3, 10), (72, 300, 65, 10), (128, 2500, 5, 40), (16, 7, 2, 10)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d-n%d-q%d-k%d" % s)
@pytest.mark.parametrize("l2", [1, 0], ids=["l2", "ip"])
@pytest.mark.parametrize("qtype", [QT_8bit, QT_fp16], ids=["sq8", "fp16"])
def test_kernel_against_model(amd, gpu, qtype, l2, shape):
    d, n, nq, k = shape
    trained, codes, xq = content(qtype, l2, d, n, nq, k)
    Dm, Im = model_search(xq, codes, qtype, trained, l2, k)
    if n > 6:
        assert Dm[0, 0] == Dm[0, 1]  # the planted ties: inside the result, and across k
        assert k >= n or model_search(xq[:1], codes, qtype, trained, l2, k + 1)[0][0, k] == Dm[0, k - 1]
    if k > n:
        assert (Im[:, n:] == -1).all() and (np.abs(Dm[:, n:]) == sq_model.FLT_MAX).all()
    same(*index_of(amd, qtype, l2, d, trained, codes).search(xq, k), Dm, Im)


@pytest.mark.parametrize("kind", ["range", "batch"])
@pytest.mark.parametrize("l2", [1, 0], ids=["l2", "ip"])
def test_selector(amd, gpu, l2, kind):
    trained, codes, xq = content(QT_8bit, l2, 72, 300, 65, 10)
    if kind == "range":
        sel, rows = amd.IDSelectorRange(10, 200), np.arange(10, 200)
    else:
        rows = np.sort(np.random.default_rng(5).permutation(300)[:40])
        sel = amd.IDSelectorBatch(rows)
    idx = index_of(amd, QT_8bit, l2, 72, trained, codes)
    D, I = idx.search(xq, 10, params=amd.SearchParametersIVF(sel=sel))
    same(D, I, *model_search(xq, codes, QT_8bit, trained, l2, 10, rows))


@pytest.mark.parametrize("l2", [1, 0], ids=["l2", "ip"])
def test_non_finite_codes(amd, gpu, l2):
    trained, codes, xq = content(QT_fp16, l2, 16, 70, 3, 10)
    half = codes.copy().view("<f2")
    half[5, 3], half[20, 0], half[40, 9] = np.inf, -np.inf, np.nan
    codes = half.view(np.uint8)
    same(*index_of(amd, QT_fp16, l2, 16, trained, codes).search(xq, 10),
         *model_search(xq, codes, QT_fp16, trained, l2, 10))


def test_query_chunk_boundary(amd, gpu):
    """70 000 rows x 1000 queries are 280 MB of dense rows: two chunks, the
    first of (2^26 // 70000) // 64 * 64 = 896 queries."""
    trained, codes, xq = content(QT_8bit, 1, 8, 70000, 1000, 10)
    D, I = index_of(amd, QT_8bit, 1, 8, trained, codes).search(xq, 10)
    qs = [0, 895, 896, 958, 999]
    same(D[qs], I[qs], *model_search(xq[qs], codes, QT_8bit, trained, 1, 10))


def test_remove_ids_then_search_and_reconstruct(amd, gpu):
    trained, codes, xq = content(QT_8bit, 1, 40, 65, 3, 10)
    idx = index_of(amd, QT_8bit, 1, 40, trained, codes)
    gone = np.array([0, 7, 8, 33, 64])
    assert idx.remove_ids(amd.IDSelectorBatch(gone)) == 5 and idx.ntotal == 60
    left = np.delete(codes, gone, axis=0)
    assert np.array_equal(idx.codes, left)
    same(*idx.search(xq, 10), *model_search(xq, left, QT_8bit, trained, 1, 10))
    idx.reset()
    assert idx.ntotal == 0 and (idx.search(xq, 2)[1] == -1).all()
    # ScalarQuantizer::decode of all 256 codes under 8 (vmin, vdiff) pairs
    fx = np.load(os.path.join(HERE, "golden", "ref_mutation.npz"))
    tab = amd.IndexScalarQuantizer(8, QT_8bit)
    tab.set_content(np.concatenate([fx["sq_vmin"], fx["sq_vdiff"]]),
                    np.repeat(np.arange(256, dtype=np.uint8)[:, None], 8, axis=1))
    assert np.array_equal(tab.reconstruct_n(0, 256).view(np.uint32), fx["sq_decode"])
    assert np.array_equal(tab.reconstruct(200).view(np.uint32), fx["sq_decode"][200])
