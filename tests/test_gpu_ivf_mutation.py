"""GPU: searches after remove_ids / update_vectors, search_and_reconstruct and
its gather-and-decode kernel.

* Against the reference-run fixtures (tests/golden/ref_mutation*,
  scripts/make_golden_mutation.py), bit for bit: a search, the same search
  again (the captured graph replays), a mutation of the host lists, the search
  again — it must give the reference's post-mutation result, so the arena was
  uploaded again and the graph retired.
* kern::ivf_reconstruct_pairs against the host reconstruct_from_offset on
  every row of small indexes built here, at the shapes where the kernel takes
  another path (see SHAPES), bit for bit: both decode the same codes with the
  same rounded operations.
"""
import ctypes

import numpy as np
import pytest

from mutation_data import TAGS, assert_lists, fixtures, map_pairs, path, selector

pytestmark = pytest.mark.gpu
NPROBE = 4


@pytest.fixture(scope="module")
def fx():
    return fixtures()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def load(amd, tag):
    idx = amd.read_index(path(tag))
    idx.nprobe = NPROBE
    return idx


def check_search(idx, fx, tag, prefix, ks, first=None):
    xq = fx[f"{tag}_xq"]
    for k in ks:
        D, I = idx.search(xq, k)
        Dr, Ir = fx[f"{tag}_{prefix}_k{k}_D"], fx[f"{tag}_{prefix}_k{k}_I"]
        bad = np.nonzero((I != Ir).any(axis=1))[0]
        assert bad.size == 0, f"{tag} {prefix} k={k}: {bad.size} queries differ, first " \
                              f"{bad[:3]}: {I[bad[0]][:8]} vs {Ir[bad[0]][:8]}"
        assert np.array_equal(bits(D), bits(Dr)), f"{tag} {prefix} k={k}: distances differ"
        # (the generator asserts the change at k = 10: at least half the queries;
        # the nearest neighbour alone may survive a mutation)
        if first is not None and k == 10:
            changed = (I != first[k][1]).any(axis=1).mean()
            assert changed >= (0.5 if prefix.startswith("rm") else 1 / 32), \
                f"the mutation changed {changed:.2f} of the queries"


@pytest.mark.parametrize("how", ["range", "batch", "array", "hash"])
@pytest.mark.parametrize("tag", TAGS)
def test_search_after_remove_ids(gpu, amd, fx, tag, how):
    idx = load(amd, tag)
    xq = fx[f"{tag}_xq"]
    first = {k: idx.search(xq, k) for k in (1, 10)}
    for k in (1, 10):  # the same call again: the graph replays
        D, I = idx.search(xq, k)
        assert np.array_equal(I, first[k][1]) and np.array_equal(bits(D), bits(first[k][0]))
    if how == "hash":
        idx.set_direct_map_type(amd.DIRECT_MAP_HASHTABLE)
    nrm = idx.remove_ids(selector(amd, fx, tag, how))
    assert nrm == int(fx[f"{tag}_rm_{how}_count"][0])
    check_search(idx, fx, tag, f"rm_{how}", (1, 10) if how == "hash" else (1, 10, 100), first)
    assert_lists(idx, fx, f"{tag}_rm_{how}")


@pytest.mark.parametrize("kind", ["array", "hash"])
@pytest.mark.parametrize("tag", TAGS)
def test_search_after_update_vectors(gpu, amd, fx, tag, kind):
    idx = load(amd, tag)
    xq = fx[f"{tag}_xq"]
    first = {k: idx.search(xq, k) for k in (1, 10)}
    for k in (1, 10):
        D, I = idx.search(xq, k)
        assert np.array_equal(I, first[k][1])
    idx.set_direct_map_type(amd.DIRECT_MAP_ARRAY if kind == "array" else amd.DIRECT_MAP_HASHTABLE)
    idx.update_vectors(fx[f"{tag}_upd_ids"], fx[f"{tag}_upd_x"])
    assert idx.ntotal == 2000
    assert_lists(idx, fx, f"{tag}_upd_{kind}")
    assert np.array_equal(map_pairs(idx, range(2000)), fx[f"{tag}_upd_{kind}_map"])
    # (the first 16 queries are the new vectors: they find themselves now)
    check_search(idx, fx, tag, f"upd_{kind}", (1, 10), first)


def test_c_flat_update_vectors(gpu, amd, fx):
    """faiss_IndexIVFFlat_update_vectors (the reference's C entry point) gives
    the recorded lists, like the class-independent form."""
    idx = load(amd, "flat")
    idx.make_direct_map(True)
    ids = np.ascontiguousarray(fx["flat_upd_ids"], dtype=np.int64)
    x = np.ascontiguousarray(fx["flat_upd_x"], dtype=np.float32)
    rc = amd.lib().faiss_IndexIVFFlat_update_vectors(
        idx.h, len(ids), ids.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, amd.lib().faiss_get_last_error()
    assert_lists(idx, fx, "flat_upd_array")
    assert np.array_equal(map_pairs(idx, range(2000)), fx["flat_upd_array_map"])


def test_update_vectors_needs_a_map(gpu, amd, fx):
    idx = load(amd, "flat")
    with pytest.raises(amd.FaissError):
        idx.update_vectors(fx["flat_upd_ids"], fx["flat_upd_x"])
    idx.make_direct_map(True)
    with pytest.raises(amd.FaissError, match="cannot have array direct map and add with ids"):
        idx.add_with_ids(fx["flat_upd_x"], fx["flat_upd_ids"])
    idx.add(fx["flat_upd_x"][:3])  # sequential ids keep the Array map
    assert idx.ntotal == 2003 and idx.direct_map_get(2002)[1] >= 0
    assert np.array_equal(bits(idx.reconstruct(2001)), bits(fx["flat_upd_x"][1]))


@pytest.mark.parametrize("tag", TAGS)
def test_search_and_reconstruct_fixture(gpu, amd, fx, tag):
    idx = load(amd, tag)
    xq = fx[f"{tag}_xq"][:16]
    D, I, R = idx.search_and_reconstruct(xq, 5)
    assert np.array_equal(I, fx[f"{tag}_sar_I"])
    assert np.array_equal(bits(D), bits(fx[f"{tag}_sar_D"]))
    assert np.array_equal(bits(R), fx[f"{tag}_sar_R"])
    # nprobe 1, k beyond the probed list: padded slots
    k = int(fx[f"{tag}_pad_k"][0])
    D, I, R = idx.search_and_reconstruct(fx[f"{tag}_pad_xq"], k, amd.SearchParametersIVF(nprobe=1))
    Ir = fx[f"{tag}_pad_I"]
    assert (Ir == -1).any() and np.array_equal(I, Ir)
    assert np.array_equal(bits(D), bits(fx[f"{tag}_pad_D"]))
    assert np.array_equal(bits(R), fx[f"{tag}_pad_R"])
    assert (bits(R)[Ir == -1] == 0xFFFFFFFF).all()


# ---------------------------------------------------------------- the kernel
class Dev:
    """hipMalloc'd buffers for the device-pointer entry points."""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.ptrs = []

    def put(self, a):
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(a.nbytes, 4))) == 0
        self.ptrs.append(p)
        if a.nbytes:
            assert self.hip.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p),
                                      ctypes.c_size_t(a.nbytes), 1) == 0
        return p

    def get(self, p, a):
        assert self.hip.hipDeviceSynchronize() == 0
        if a.nbytes:
            assert self.hip.hipMemcpy(a.ctypes.data_as(ctypes.c_void_p), p,
                                      ctypes.c_size_t(a.nbytes), 2) == 0
        return a

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def pairs_on_device(idx, pairs):
    """kern::ivf_reconstruct_pairs on `pairs` [n] -> (ids [n], rows [n][d])."""
    dev = Dev()
    try:
        lab = np.ascontiguousarray(pairs, dtype=np.int64)
        R = np.full((len(lab), idx.d), 0x12345678, np.uint32).view(np.float32)
        pl, pr = dev.put(lab), dev.put(R)
        idx.reconstruct_pairs_device(len(lab), pl.value, pr.value)
        return dev.get(pl, np.empty_like(lab)), dev.get(pr, R)
    finally:
        dev.free()


LIST_SIZES = [0, 1, 63, 65, 64]  # the last list ends on the arena's last row


def build(amd, kind, d, by_residual, M=0, nbits=8):
    """An index of 5 lists holding LIST_SIZES rows, on a flat quantizer of 5
    far-apart centroids (so every vector lands in the list it was made for)."""
    rng = np.random.default_rng(1000 * d + 10 * nbits + by_residual)
    nl = len(LIST_SIZES)
    cent = (rng.standard_normal((nl, d)) + 40.0 * np.arange(nl)[:, None]).astype(np.float32)
    q = amd.IndexFlatL2(d)
    q.add(cent)

    def around(sizes):
        return np.concatenate([cent[l] + rng.standard_normal((n, d)).astype(np.float32)
                               for l, n in enumerate(sizes)]).astype(np.float32)
    if kind == "flat":
        idx = amd.IndexIVFFlat(q, d, nl)
    elif kind == "pq":
        idx = amd.IndexIVFPQ(q, d, nl, M, nbits)
        idx.by_residual = by_residual
    else:
        idx = amd.IndexIVFScalarQuantizer(q, d, nl, amd.QT_8bit if kind == "sq8" else amd.QT_fp16,
                                          amd.METRIC_L2, by_residual)
    idx.train(around([120] * nl))
    idx.add(around(LIST_SIZES))
    assert [idx.get_list_size(l) for l in range(nl)] == LIST_SIZES
    return idx


SHAPES = (  # kind, d, by_residual, M, nbits
    # d = 1028: rows of 4112 bytes, staged in two passes (4096 + 16)
    [("flat", d, 0, 0, 8) for d in (4, 36, 264, 1028)]
    # M * nbits = 10, 36, 45, 54, 63, 165 bits: no multiple of 8, fields straddle
    # bytes; nbits = 8 is whole bytes; 264 = 33 * 8 sub-vectors
    + [("pq", 4, 1, 2, 5), ("pq", 36, 1, 9, 4), ("pq", 36, 0, 9, 5), ("pq", 36, 1, 9, 6),
       ("pq", 36, 0, 9, 7), ("pq", 36, 1, 9, 8), ("pq", 264, 1, 33, 5), ("pq", 264, 0, 33, 8)]
    # SQ is served for d % 8 == 0 only: 8 and 264 stand in for 4 and 36
    + [("sq8", 8, 1, 0, 8), ("sq8", 264, 0, 0, 8), ("sq8", 264, 1, 0, 8),
       ("sqfp16", 8, 0, 0, 8), ("sqfp16", 264, 1, 0, 8)])


@pytest.mark.parametrize("kind,d,by_residual,M,nbits", SHAPES,
                         ids=[f"{s[0]}-d{s[1]}-res{s[2]}-M{s[3]}x{s[4]}" for s in SHAPES])
def test_kernel_every_row(gpu, amd, kind, d, by_residual, M, nbits):
    idx = build(amd, kind, d, bool(by_residual), M, nbits)
    pairs, ids, rows = [], [], []
    for l, n in enumerate(LIST_SIZES):
        lid = idx.list_ids(l)
        for o in range(n):
            pairs.append((l << 32) | o)
            ids.append(int(lid[o]))
            rows.append(idx.reconstruct_from_offset(l, o))
    pairs, ids, rows = np.array(pairs, np.int64), np.array(ids, np.int64), np.stack(rows)
    # every row at once (193 slots: more than one work group, a partial last one)
    I, R = pairs_on_device(idx, pairs)
    assert np.array_equal(I, ids)
    assert np.array_equal(bits(R), bits(rows)), \
        f"rows differing: {np.nonzero((bits(R) != bits(rows)).any(axis=1))[0][:8]}"
    # n = 1: the arena's last row (list 4 fills its 64-row tile to the end)
    rb, arena_rows = idx.debug_rows(0)
    assert arena_rows == 64 * 5  # tiles of 64 rows: lists of 0, 1, 63, 65 (two tiles), 64
    I, R = pairs_on_device(idx, pairs[-1:])
    assert I[0] == ids[-1] and np.array_equal(bits(R[0]), bits(rows[-1]))
    # n = 65 with negative labels and pairs that name no row mixed in
    sel = np.arange(0, 65) * 2
    mixed = pairs[sel].copy()
    mixed[[3, 40]] = -1
    mixed[7] = (1 << 32) | 1          # list 1 has one row
    mixed[9] = (0 << 32) | 0          # list 0 is empty
    mixed[11] = (len(LIST_SIZES) << 32)  # no such list
    none = np.array([3, 40, 7, 9, 11])
    I, R = pairs_on_device(idx, mixed)
    want_i, want_r = ids[sel].copy(), bits(rows[sel]).copy()
    want_i[none], want_r[none] = -1, 0xFFFFFFFF
    assert np.array_equal(I, want_i) and np.array_equal(bits(R), want_r)
    # a batch that is all -1
    I, R = pairs_on_device(idx, np.full(65, -1, np.int64))
    assert (I == -1).all() and (bits(R) == 0xFFFFFFFF).all()


@pytest.mark.parametrize("tag", ["flat", "pq12x5", "sq8"])
def test_device_entry_equals_host_entry(gpu, amd, fx, tag):
    idx = load(amd, tag)
    xq = np.ascontiguousarray(fx[f"{tag}_xq"][:13])
    n, k, d = len(xq), 5, idx.d
    D, I, R = idx.search_and_reconstruct(xq, k)
    dev = Dev()
    try:
        px = dev.put(xq)
        pd = dev.put(np.zeros((n, k), np.float32))
        pi = dev.put(np.zeros((n, k), np.int64))
        pr = dev.put(np.zeros((n, k, d), np.float32))
        idx.search_and_reconstruct_device(n, px.value, k, pd.value, pi.value, pr.value)
        D2 = dev.get(pd, np.empty((n, k), np.float32))
        I2 = dev.get(pi, np.empty((n, k), np.int64))
        R2 = dev.get(pr, np.empty((n, k, d), np.float32))
    finally:
        dev.free()
    assert np.array_equal(I2, I) and np.array_equal(bits(D2), bits(D))
    assert np.array_equal(bits(R2), bits(R))
    assert np.array_equal(I, fx[f"{tag}_sar_I"][:13])
