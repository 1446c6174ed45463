"""IndexBinaryFlat / IndexBinaryIVF on the GPU against tests/binary_model.py
(pinned to the reference by tests/test_binary_model.py): D and I exactly equal.

Flat shapes: code sizes 1, 4, 5 (pads), 32 (dwordx4 rows), 36 (9 dwords), 68 (17
dwords: one 16-dword chunk plus one, dword loads), 80 (20 dwords: dwordx4 rows
over two chunks); 1, 63, 65 rows, 2049 rows (two slabs) and 1000 rows of 8 bits
(only 9 distances exist); 1 and 17 queries (a tile plus one); k around the
in-scan select's limit of 32, and k = ntotal + 3 (pads).  d = 65536, the widest
served: the 8-query tile of the flat scan, alone and as the IVF quantizer.
IVF: lists of 0, 1, 63, 65 and 300 rows (one wave per probe) or 1100 (four),
shuffled ids, so arrival order and id order differ."""
import os

import numpy as np
import pytest

import binary_model as bm

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_binary")


def check(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


SHAPES = [(cs, n) for cs in (1, 4, 5, 32, 36, 68, 80) for n in (1, 63, 65, 2049)] + [(1, 1000)]


@pytest.mark.parametrize("code_size,ntotal", SHAPES)
def test_flat(amd, code_size, ntotal):
    rng = np.random.default_rng(100 * code_size + ntotal)
    xb = rng.integers(0, 256, (ntotal, code_size), dtype=np.uint8)
    xb[ntotal // 2:] = xb[:ntotal - ntotal // 2]  # duplicate rows: ties at every width
    xq = rng.integers(0, 256, (17, code_size), dtype=np.uint8)
    idx = amd.IndexBinaryFlat(8 * code_size)
    idx.add(xb)
    for k in sorted({1, 32, 33, 64, 65, min(ntotal + 3, 2048)}):
        want = bm.flat_search(xb, xq, k)
        for nq in (1, 17):
            for heap in (True, False):
                idx.use_heap = heap
                check(idx.search(xq[:nq], k), (want[0][:nq], want[1][:nq]), (k, nq, heap))


@pytest.mark.parametrize("use_heap", [True, False])
@pytest.mark.parametrize("long_list", [300, 1100])
def test_ivf(amd, long_list, use_heap):
    lens = [0, 1, 63, 65, long_list]
    rng = np.random.default_rng(long_list)
    cs = 8
    cent = rng.integers(0, 256, (len(lens), cs), dtype=np.uint8)
    assert bm.hamming(cent, cent)[np.triu_indices(len(lens), 1)].min() > 8
    rows = np.repeat(np.arange(len(lens)), lens)
    flips = np.zeros((len(rows), cs), np.uint8)  # up to three flipped bits per row
    for _ in range(3):
        bit = rng.integers(0, 8 * cs + 8, len(rows))  # (past the code: no flip)
        ok = bit < 8 * cs
        flips[np.flatnonzero(ok), bit[ok] >> 3] ^= (1 << (bit[ok] & 7)).astype(np.uint8)
    xb = cent[rows] ^ flips
    order = rng.permutation(len(rows))
    xb = xb[order]
    ids = rng.permutation(len(rows)).astype(np.int64) + 7
    q = amd.IndexBinaryFlat(8 * cs)
    q.add(cent)
    idx = amd.IndexBinaryIVF(q, 8 * cs, len(lens))
    idx.is_trained = True
    idx.add_with_ids(xb, ids)
    idx.use_heap = use_heap
    model = bm.IVFModel(cent, xb, ids)
    assert sorted(len(l) for l in model.lists) == sorted(lens)
    xq = np.concatenate([cent, xb[:4] ^ np.uint8(1)])
    for nprobe in (1, 3, len(lens) + 2):
        for max_codes in (0, 64):
            idx.nprobe, idx.max_codes = nprobe, max_codes
            for k in (1, 10, 33, 70):
                want = model.search(xq, k, nprobe, use_heap, max_codes)
                check(idx.search(xq, k), want, (nprobe, max_codes, k))
    # per-call parameters, and the probes given by the caller
    idx.nprobe, idx.max_codes = 1, 0
    want = model.search(xq, 10, 3, use_heap, 64)
    check(idx.search(xq, 10, params=amd.SearchParametersIVF(nprobe=3, max_codes=64)), want, "sp")
    assign = np.array([(model.probes(x, 3) + [-1, -1])[:3] for x in xq], np.int64)
    idx.nprobe = 3
    check(idx.search_preassigned(xq, 10, assign), model.search(xq, 10, 3, use_heap), "pre")


@pytest.mark.parametrize("tag", ["flat_heap", "flat_count", "ivf_heap", "ivf_count",
                                 "ivf_heap_mc64", "ivf_count_mc64"])
def test_reference_fixtures(amd, tag):
    ref = np.load(os.path.join(GOLDEN, "ref_binary.npz"))
    heap, nprobe, mc = (int(v) for v in ref[tag + "_cfg"])
    idx = amd.read_index_binary(os.path.join(GOLDEN, tag.split("_")[0] + ".faiss"))
    idx.use_heap = bool(heap)
    if nprobe:
        idx.nprobe, idx.max_codes = nprobe, mc
    check(idx.search(ref["xq"], int(ref["k"])), (ref[tag + "_D"], ref[tag + "_I"]), tag)


@pytest.mark.parametrize("k", [1, 32, 33])
def test_widest_codes(amd, k):
    """d = 65536 bits (2048 dwords a row): k <= 32 runs the 8-query tile."""
    cs, n, nlist = 65536 // 8, 70, 3
    rng = np.random.default_rng(k)
    xb = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    xb[n // 2:] = xb[:n - n // 2]
    xq = rng.integers(0, 256, (9, cs), dtype=np.uint8)
    flat = amd.IndexBinaryFlat(8 * cs)
    flat.add(xb)
    check(flat.search(xq, k), bm.flat_search(xb, xq, k), "flat")
    quant = amd.IndexBinaryFlat(8 * cs)
    quant.add(xb[:nlist])
    ivf = amd.IndexBinaryIVF(quant, 8 * cs, nlist)
    ivf.is_trained = True
    ids = rng.permutation(n).astype(np.int64)
    ivf.add_with_ids(xb, ids)
    ivf.nprobe = 2
    check(ivf.search(xq, k), bm.IVFModel(xb[:nlist], xb, ids).search(xq, k, 2), "ivf")


def test_train(amd):
    """train(): bits -> +-1 floats, k-means, centroids thresholded at 0.  Two
    well separated clusters (a pattern with up to 4 of 64 bits flipped; 2-means
    splits two such blobs from any start) must come back as the patterns
    themselves, in either order; then add and search run against the model over
    those centroids."""
    rng = np.random.default_rng(5)
    cs, nlist, per = 8, 2, 100
    pat = rng.integers(0, 256, (nlist, cs), dtype=np.uint8)
    assert bm.hamming(pat, pat)[np.triu_indices(nlist, 1)].min() > 16
    xb = np.repeat(pat, per, axis=0)
    for _ in range(4):
        bit = rng.integers(0, 8 * cs, len(xb))
        xb[np.arange(len(xb)), bit >> 3] ^= (1 << (bit & 7)).astype(np.uint8)
    xb = xb[rng.permutation(len(xb))]
    idx = amd.index_binary_factory(8 * cs, f"BIVF{nlist}")
    assert not idx.is_trained
    idx.train(xb)
    assert idx.is_trained and idx.quantizer.ntotal == nlist and idx.quantizer.is_trained
    cent = np.stack([idx.quantizer.reconstruct(i) for i in range(nlist)])
    assert sorted(map(bytes, cent)) == sorted(map(bytes, pat))
    idx.add(xb)
    model = bm.IVFModel(cent, xb, np.arange(len(xb)))
    for nprobe in (1, 2):
        idx.nprobe = nprobe
        check(idx.search(xb[:7], 10), model.search(xb[:7], 10, nprobe), nprobe)
