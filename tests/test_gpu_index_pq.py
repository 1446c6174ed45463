"""IndexPQ's full scan (csrc/kernels_pq_flat.hip) on the GPU.

Bound of test 1.  A distance is sum_m t_m, t_m a table entry of dsub terms.
An fp32 sum of n terms evaluated in any order is within (n - 1) u |terms| of
the exact sum to first order (u = 2^-24); each L2 term (q - y)^2 carries two
more roundings, an IP term q y one.  So an entry is within (dsub + 1) u of its
terms' magnitude sum, the code sum of M entries adds (M - 1) u (its leading
0 + t_0 is exact), and |D - D64| <= (M + dsub) u sum|terms| to first order;
the test allows 2 (M + dsub + 2) u sum|terms|.  Two rows can swap only when
their float64 distances are closer than the sum of their bounds, so a query
is compared id by id when every gap of its float64 top k + 1 exceeds twice
the largest bound in it; the seeds are chosen (on the CPU, from the float64
values alone) so that no query is set aside, and the test asserts that.

Tie order.  The reference heap admits strictly better keys only and rows
arrive in id order, so of equal distances the lowest ids survive; heap_reorder
lists L2 ties by ascending id and inner-product ties by descending id (CMin
orders by (value, id) and is emptied from its smallest).  The recorded
reference results (scripts/make_golden_index_pq.py) pin both."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_index_pq")
U = 2.0 ** -24
SEED = 62


def unpack(codes, M, nbits):
    bits = np.unpackbits(codes, axis=1, bitorder="little")[:, :M * nbits]
    return (bits.reshape(-1, M, nbits) << np.arange(nbits)).sum(-1)


def reference(xq, cent, codes, nbits, l2):
    """float64 distances [nq][n] and the bound of the docstring."""
    M, _, dsub = cent.shape
    dec = cent[np.arange(M), unpack(codes, M, nbits)].reshape(len(codes), M * dsub).astype(np.float64)
    x = xq.astype(np.float64)[:, None, :]
    terms = (x - dec[None]) ** 2 if l2 else x * dec[None]
    return terms.sum(-1), 2 * (M + dsub + 2) * U * np.abs(terms).sum(-1)


@functools.lru_cache(maxsize=None)
def make(M, nbits, d, n, nq, l2, seed=SEED):
    rng = np.random.default_rng([seed, M, nbits, d, n, nq, l2])
    cent = rng.standard_normal((M, 1 << nbits, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, (n, (M * nbits + 7) // 8), dtype=np.uint8)
    if M == 1:  # one byte per row: distinct codes, or rows tie exactly
        codes = rng.permutation(256)[:n].astype(np.uint8).reshape(-1, 1)
    if (M * nbits) % 8:
        codes[:, -1] &= (1 << (M * nbits) % 8) - 1
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    return cent, codes, xq


def index_of(amd, cent, codes, nbits, l2):
    M, _, dsub = cent.shape
    idx = amd.IndexPQ(M * dsub, M, nbits, amd.METRIC_L2 if l2 else amd.METRIC_INNER_PRODUCT)
    idx.set_content(cent, codes)
    return idx


def check(D, I, D64, bound, k, l2):
    """D within the bound of the float64 value of the row it names, ids in the
    float64 order; returns the number of queries set aside."""
    key = D64 if l2 else -D64
    n = key.shape[1]
    order = np.argsort(key, axis=1, kind="stable")
    kk = min(k, n)
    aside = 0
    for q in range(len(D)):
        top = order[q, :min(kk + 1, n)]
        print(f"q{q}: max |D - D64| / bound = "
              f"{np.max(np.abs(D[q, :kk] - D64[q, I[q, :kk]]) / bound[q, I[q, :kk]], initial=0):.3f}")
        assert (I[q, kk:] == -1).all() and (D[q, kk:] == (1 if l2 else -1) * np.float32(3.4028235e38)).all()
        assert (np.abs(D[q, :kk] - D64[q, I[q, :kk]]) <= bound[q, I[q, :kk]]).all()
        if (np.diff(key[q, top]) <= 2 * bound[q, top].max(initial=0)).any():
            aside += 1
            continue
        assert np.array_equal(I[q, :kk], order[q, :kk])
    return aside


BASE = dict(M=8, nbits=8, d=32, n=257, nq=5, k=10, l2=1)
CASES = ([dict(nq=v) for v in (1, 3, 4, 9)] +
         [dict(n=v) for v in (0, 1, 9, 255, 256, 3100)] +
         [dict(k=v) for v in (1, 40, 257)] +
         [dict(M=1, d=4, n=200), dict(M=5, nbits=5, d=20), dict(M=12, nbits=6, d=48),
          dict(M=16, nbits=4, d=32), dict(M=32, d=64), dict(M=64, d=128), dict(M=96, d=96),
          dict(M=256, d=256), dict(l2=0), dict(l2=0, M=12, nbits=6, d=48), {}])


@pytest.mark.parametrize("over", CASES, ids=lambda o: "-".join(f"{a}{b}" for a, b in o.items()) or "base")
def test_kernel_against_float64(amd, gpu, over):
    c = dict(BASE, **over)
    cent, codes, xq = make(c["M"], c["nbits"], c["d"], c["n"], c["nq"], c["l2"])
    D64, bound = reference(xq, cent, codes, c["nbits"], c["l2"])
    D, I = index_of(amd, cent, codes, c["nbits"], c["l2"]).search(xq, c["k"])
    assert check(D, I, D64, bound, c["k"], c["l2"]) == 0


def test_ties_straddle_slab_and_k(amd, gpu):
    """Sixteen copies of the best row across the boundary of the first two
    slabs (1280 rows each at this shape): the ten lowest ids, ascending."""
    cent, codes, xq = make(8, 8, 32, 3100, 1, 1)
    codes = codes.copy()
    D64, _ = reference(xq, cent, codes, 8, 1)
    best = int(np.argmin(D64[0]))
    codes[1275:1291] = codes[best]
    want = np.sort(np.append(np.arange(1275, 1291), best))[:10]
    D, I = index_of(amd, cent, codes, 8, 1).search(xq, 10)
    assert np.array_equal(I[0], want) and (D[0] == D[0, 0]).all()


@pytest.mark.parametrize("tag", ["pq8x8_l2", "pq8x8_ip", "pq16x8_l2", "pq5x5_l2", "pq12x6_ip",
                                 "pq16x4_l2", "pq2x8_dsub16_l2"])
def test_reference_fixtures(amd, gpu, tag):
    idx = amd.read_index(os.path.join(GOLDEN, tag + ".faiss"))
    f = np.load(os.path.join(GOLDEN, tag + ".npz"))
    D, I = idx.search(f["xq"], 10)
    if "dsub16" not in tag:
        assert np.array_equal(I, f["I"])
        assert np.array_equal(D.view(np.uint32), f["D"].view(np.uint32))
        return
    info = idx.pq_info()
    D64, bound = reference(f["xq"], idx.pq_centroids, idx.codes, info["nbits"], idx.metric_type)
    for Dx, Ix in ((D, I), (f["D"], f["I"])):
        assert (np.abs(Dx - np.take_along_axis(D64, Ix, 1)) <= np.take_along_axis(bound, Ix, 1)).all()


@functools.lru_cache(maxsize=None)
def trained(amd):
    rng = np.random.default_rng(SEED)
    xb = rng.standard_normal((1500, 32)).astype(np.float32)
    xq = rng.standard_normal((9, 32)).astype(np.float32)
    idx = amd.index_factory(32, "PQ8x6")
    idx.train(xb)
    idx.add(xb)
    return idx, xb, xq


def test_interface_train_add_search_io(amd, gpu, tmp_path):
    idx, xb, xq = trained(amd)
    assert idx.is_trained and idx.ntotal == 1500
    amd.indexPQ_stats(reset=True)
    D, I = idx.search(xq, 10)
    assert amd.indexPQ_stats() == dict(nq=9, ncode=9 * 1500)
    D64, bound = reference(xq, idx.pq_centroids, idx.codes, 6, 1)
    rec = idx.reconstruct_n(0, 1500)
    assert np.array_equal(rec, idx.pq_centroids[np.arange(8), unpack(idx.codes, 8, 6)].reshape(1500, 32))
    check(D, I, D64, bound, 10, 1)
    # a query alone and in the batch of 9: the same bits
    for q in (0, 4, 8):
        D1, I1 = idx.search(xq[q:q + 1], 10)
        assert np.array_equal(I1[0], I[q]) and np.array_equal(D1.view(np.uint32)[0], D.view(np.uint32)[q])
    amd.write_index(idx, str(tmp_path / "a.faiss"))
    idx2 = amd.read_index(str(tmp_path / "a.faiss"))
    amd.write_index(idx2, str(tmp_path / "b.faiss"))
    assert (tmp_path / "a.faiss").read_bytes() == (tmp_path / "b.faiss").read_bytes()
    D2, I2 = idx2.search(xq, 10)
    assert np.array_equal(I2, I) and np.array_equal(D2.view(np.uint32), D.view(np.uint32))


def test_interface_compositions(amd, gpu):
    idx, xb, xq = trained(amd)
    # "PQ..,RFlat": the base's 20 candidates re-ranked by exact distance
    rf = amd.index_factory(32, "PQ8x6,RFlat")
    rf.train(xb)
    rf.add(xb)
    rf.k_factor = 2
    Dr, Ir = rf.search(xq, 10)
    _, Ib = rf.base_index.search(xq, 20)
    ex = ((xq[:, None, :].astype(np.float64) - xb[Ib].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(Ir, np.take_along_axis(Ib, np.argsort(ex, axis=1, kind="stable")[:, :10], 1))
    # a filled rotation in front: the sub-index's answer on the rotated queries
    A = np.linalg.qr(np.random.default_rng(SEED).standard_normal((32, 32)))[0].astype(np.float32)
    lt = amd.LinearTransform(32, 32, A=A)
    pt = amd.IndexPreTransform(lt, idx)
    Dp, Ip = pt.search(xq, 10)
    Ds, Is = idx.search(lt.apply(xq), 10)
    assert np.array_equal(Ip, Is) and np.array_equal(Dp.view(np.uint32), Ds.view(np.uint32))
