"""GPU: IndexHNSW honours SearchParametersHNSW::check_relative_distance /
bounded_queue / sel and the index-level hnsw.check_relative_distance /
hnsw.search_bounded_queue, alone and as an IVF coarse quantizer.

Every case of tests/golden/ref_hnsw_params.npz (reference runs, see
scripts/make_golden_hnsw_params.py) must come back bit-equal — D, I and the
four HNSWStats deltas — through the host search, search_device (int64 labels)
and the IVF path; one IVF case also through IndexShardsIVF.  Shapes without a
fixture are held to tests/hnsw_params_model.py, which
tests/test_hnsw_params_model.py pins to the same fixtures.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hnsw_params_model as hm  # noqa: E402
from test_hnsw_params_model import FILES, FX, jobs  # noqa: E402

pytestmark = pytest.mark.gpu
IVF_FILE = os.path.join(HERE, "golden", "ref_full", "hnswivf.faiss")


def make_sel(amd, spec):
    if spec == "none":
        return None
    p = spec.split(":")
    if p[0] == "range":
        return amd.IDSelectorRange(int(p[1]), int(p[2]))
    ids = (int(p[1]) + int(p[2]) * np.arange(int(p[3]))).astype(np.int64)
    b = amd.IDSelectorBatch(ids)
    if p[0] == "batch":
        return b
    n = amd.IDSelectorNot(b)
    n._keep = b
    return n


def search_dev(idx, xq, k, params):
    """Index::search_device with params on hipMalloc'd copies; host (D, I int64)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    xq = np.ascontiguousarray(xq, dtype=np.float32)
    n = xq.shape[0]
    ptrs = []
    for nbytes in (xq.nbytes, n * k * 4, n * k * 8):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(nbytes, 4))) == 0
        ptrs.append(p)
    px, pd, pi = ptrs
    try:
        hip.hipMemcpy(px, xq.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(xq.nbytes), 1)
        idx.search_device(n, px.value, k, pd.value, pi.value, params=params)
        assert hip.hipDeviceSynchronize() == 0
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        hip.hipMemcpy(D.ctypes.data_as(ctypes.c_void_p), pd, ctypes.c_size_t(D.nbytes), 2)
        hip.hipMemcpy(I.ctypes.data_as(ctypes.c_void_p), pi, ctypes.c_size_t(I.nbytes), 2)
    finally:
        for p in ptrs:
            hip.hipFree(p)
    idx.fold_device_stats()
    return D, I


def apply(amd, hidx, job):
    """Set up a fixture case on the IndexHNSW hidx; returns its
    SearchParametersHNSW (None: the index-level values act)."""
    name, k, how, ef, chk, bnd, sel, _ = job
    hidx.efSearch, hidx.check_relative_distance, hidx.search_bounded_queue = 16, True, True
    if how == "params":
        return amd.SearchParametersHNSW(ef, chk, bnd, make_sel(amd, sel))
    if how == "index":
        hidx.efSearch, hidx.check_relative_distance, hidx.search_bounded_queue = ef, chk, bnd
        return None
    hidx.check_relative_distance = hidx.search_bounded_queue = False  # "cleared"
    return amd.SearchParametersHNSW()


def stats(amd):
    hs = amd.cvar.hnsw_stats
    return [hs.n1, hs.n2, hs.ndis, hs.nhops]


def check(amd, key, run):
    amd.cvar.hnsw_stats.reset()
    D, I = run()
    st = stats(amd)
    assert I.dtype == np.int64
    np.testing.assert_array_equal(I, FX[key + "_I"], err_msg=key)
    np.testing.assert_array_equal(D, FX[key + "_D"], err_msg=key)
    assert st == [int(v) for v in FX[key + "_st"]], (key, st)


@pytest.fixture(scope="module")
def indexes(amd, gpu):
    return {tag: amd.read_index(fn) for tag, fn in FILES.items()}


@pytest.mark.parametrize("path", ["host", "device", "search_stats"])
@pytest.mark.parametrize("tag", ["dup", "h24"])
def test_hnsw_params_equal_reference(amd, indexes, tag, path):
    idx = indexes[tag]
    xq = FX[f"{tag}_xq"]
    for job in jobs(tag):
        params = apply(amd, idx, job)
        if path == "host":
            check(amd, f"{tag}_{job[0]}", lambda: idx.search(xq, job[1], params=params))
        elif path == "search_stats":
            check(amd, f"{tag}_{job[0]}", lambda: idx.search_stats(xq, job[1], params)[:2])
        else:
            check(amd, f"{tag}_{job[0]}", lambda: search_dev(idx, xq, job[1], params))


@pytest.mark.parametrize("path", ["host", "device", "shards"])
def test_ivf_quantizer_params_equal_reference(amd, gpu, path):
    idx = amd.read_index(IVF_FILE)
    q = idx.quantizer
    xq = FX["ivf_xq"]
    js = jobs("ivf")
    if path == "shards":  # one case per mode through IndexShardsIVF on one device
        js = [j for j in js if j[0] in ("A_np8", "B_np8", "sel_np8", "ixB_np8")]
    assert js
    for job in js:
        sh = amd.index_ivf_to_shards(idx, 2, 1, devices=[0, 0]) if path == "shards" else None
        qp = apply(amd, sh.quantizer if sh else q, job)
        idx.nprobe = job[7]
        sp = amd.SearchParametersIVF(nprobe=job[7], quantizer_params=qp) if qp else None
        if path == "host":
            check(amd, f"ivf_{job[0]}", lambda: idx.search(xq, job[1], params=sp))
        elif path == "device":
            check(amd, f"ivf_{job[0]}", lambda: search_dev(idx, xq, job[1], sp))
        else:
            sh.nprobe = job[7]

            def run_shards():
                # (IndexShardsIVF::search leaves its quantizer's device
                # counters to the caller, like the device entry points)
                r = sh.search(xq, job[1], params=sp)
                sh.quantizer.fold_device_stats()
                return r
            check(amd, f"ivf_{job[0]}", run_shards)


def test_set_quantizer_hnsw_c_entry(amd, gpu):
    """faiss_amd_SearchParametersIVF_set_quantizer_hnsw: the three values
    without a params object of their own."""
    idx = amd.read_index(IVF_FILE)
    sp = amd.SearchParametersIVF(nprobe=100)
    amd.lib().faiss_amd_SearchParametersIVF_set_quantizer_hnsw(sp.h, 64, 1, 0)
    check(amd, "ivf_B_np100", lambda: idx.search(FX["ivf_xq"], 10, params=sp))


def test_wrong_params_type_throws(amd, indexes):
    with pytest.raises(amd.FaissError, match="params type invalid"):
        indexes["dup"].search(FX["dup_xq"], 5, params=amd.SearchParametersIVF(nprobe=2))


# ---------------------------------------------------------------- model shapes
MODES = [("A", dict(check_relative_distance=False)),
         ("B", dict(bounded_queue=False)),
         ("sel", dict()), ("selA", dict(check_relative_distance=False))]


def vs_model(amd, orc, idx, xq, k, ef, modes=MODES, device=True, member=None):
    m = hm.Model(orc, orc.HNSWGraph.from_index(idx))
    n = idx.ntotal
    if member is None:
        member = (np.arange(n) % 3) == 1
    sel_ids = np.nonzero(member)[0].astype(np.int64)
    for name, kw in modes:
        mem = member if name.startswith("sel") else None
        sel = amd.IDSelectorBatch(sel_ids) if mem is not None else None
        Dm, Im, stm = m.search(xq, k, ef, member=mem, **kw)
        params = amd.SearchParametersHNSW(ef, sel=sel, **kw)
        runs = [lambda: idx.search(xq, k, params=params)]
        if device:
            runs.append(lambda: search_dev(idx, xq, k, params))
        for run in runs:
            amd.cvar.hnsw_stats.reset()
            D, I = run()
            np.testing.assert_array_equal(I, Im, err_msg=name)
            np.testing.assert_array_equal(D, Dm, err_msg=name)
            assert stats(amd) == [int(v) for v in stm], name
    return m


@pytest.mark.parametrize("d", [4, 13, 132])
def test_odd_dimensions_equal_model(amd, orc, gpu, d):
    """d = 4 (one 4-term epilogue), 13 (ld 16, an fma tail; host search only:
    the device entry needs d % 4 == 0) and 132 (past the 4-lanes-per-row form)."""
    idx = amd.IndexHNSWFlat(d, 8)
    xb = orc.float_rand(500 * d, 900 + d).reshape(500, d)
    xb[450:] = xb[:50]
    idx.add(xb)
    xq = np.concatenate([orc.float_rand(12 * d, 901 + d).reshape(12, d), xb[:4]])
    for ef, k in ((8, 3), (40, 70)):
        vs_model(amd, orc, idx, xq, k, ef, device=d % 4 == 0)


def test_k_2048_equals_model(amd, orc, indexes):
    """k above ntotal = 1900 (padding) and above every LDS-resident heap size
    of the fast kernels; the result heap form of the sequential kernel."""
    vs_model(amd, orc, indexes["h24"], FX["h24_xq"][36:44], 2048, 16)


def test_empty_and_single_vector(amd, orc, gpu):
    idx = amd.IndexHNSWFlat(8, 8)
    xq = orc.float_rand(5 * 8, 3).reshape(5, 8)
    for kw in (dict(check_relative_distance=False), dict(bounded_queue=False),
               dict(sel=amd.IDSelectorRange(0, 4))):
        amd.cvar.hnsw_stats.reset()
        D, I = idx.search(xq, 3, params=amd.SearchParametersHNSW(4, **kw))
        assert (I == -1).all() and (D == hm.FLT_MAX).all() and stats(amd) == [0, 0, 0, 0]
    idx.add(xq[:1])
    vs_model(amd, orc, idx, xq, 3, 4, member=np.array([True]))
    vs_model(amd, orc, idx, xq, 3, 4, modes=MODES[2:], member=np.array([False]))


def test_selector_of_unreachable_rows(amd, orc, gpu):
    """A selector whose only members no traversal can reach: every row is
    padding whatever efSearch (the selector never steers the search)."""
    idx = amd.IndexHNSWFlat(8, 2)
    idx.add(orc.float_rand(600 * 8, 77).reshape(600, 8))
    g = orc.HNSWGraph.from_index(idx)
    seen, todo = {int(g.s.entry_point)}, [int(g.s.entry_point)]
    while todo:
        v = todo.pop()
        for w in g.neighbors[int(g.offsets[v]):int(g.offsets[v + 1])]:
            if w >= 0 and int(w) not in seen:
                seen.add(int(w))
                todo.append(int(w))
    member = ~np.isin(np.arange(600), sorted(seen))
    assert member.sum() >= 1
    xq = orc.float_rand(10 * 8, 78).reshape(10, 8)
    vs_model(amd, orc, idx, xq, 5, 1000, modes=MODES[2:], member=member)
    D, I = idx.search(xq, 5, params=amd.SearchParametersHNSW(
        1000, sel=amd.IDSelectorBatch(np.nonzero(member)[0].astype(np.int64))))
    assert (I == -1).all()


def test_unbounded_batch_is_chunked(amd, orc, gpu):
    """bounded_queue = false keeps 8 (min(ef, ntotal) + ntotal + 4) bytes of
    queue scratch per query, in chunks of the batch under 256 MiB: 1800
    queries of a 20000-node graph make two chunks.  The queries repeat 60
    rows, so the model runs 60."""
    d, n, ef, k, rep = 8, 20000, 16, 4, 30
    idx = amd.IndexHNSWFlat(d, 4)
    idx.add(orc.float_rand(n * d, 41).reshape(n, d))
    per_query = 8 * (min(ef, n) + n + 4)
    x60 = orc.float_rand(60 * d, 42).reshape(60, d)
    xq = np.tile(x60, (rep, 1))
    assert xq.shape[0] > (256 << 20) // per_query
    m = hm.Model(orc, orc.HNSWGraph.from_index(idx))
    Dm, Im, stm = m.search(x60, k, ef, bounded_queue=False)
    amd.cvar.hnsw_stats.reset()
    D, I = idx.search(xq, k, params=amd.SearchParametersHNSW(ef, bounded_queue=False))
    np.testing.assert_array_equal(I, np.tile(Im, (rep, 1)))
    np.testing.assert_array_equal(D, np.tile(Dm, (rep, 1)))
    assert stats(amd) == [int(v) * rep for v in stm]
