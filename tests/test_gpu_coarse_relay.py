"""GPU parity of the coarse re-rank's relayed chain (k_coarse_rerank).

The re-rank evaluates <x, c> with four lanes per candidate row: every lane
fetches its segment of the row at once and the accumulator is handed from
lane to lane in chain order, so the fmaf sequence on the live accumulator is
the one the oracle runs.  Every comparison here is therefore bit-exact.
"""
import re

import numpy as np
import pytest

from conftest import assert_same_results, rand

pytestmark = pytest.mark.gpu

NQ_RAND, NQ_ROWS = 180, 20


def make_flat(amd, orc, d, ny, metric, seed=41):
    """Random base with 40 duplicated rows (exact ties at the k boundary);
    ~200 queries, 20 of them equal to database rows."""
    y = rand(orc, ny, d, seed)
    y[ny // 2: ny // 2 + 40] = y[:40]
    x = np.ascontiguousarray(np.concatenate([rand(orc, NQ_RAND, d, seed + 1), y[:NQ_ROWS]]))
    idx = amd.IndexFlat(d, metric)
    idx.add(y)
    return idx, x, y


@pytest.fixture(scope="module")
def flat_cases(amd, orc, gpu):
    """(d, metric) -> (index, queries, base), built once per module."""
    cache = {}

    def get(d, metric, ny):
        key = (d, metric, ny)
        if key not in cache:
            cache[key] = make_flat(amd, orc, d, ny, metric)
        return cache[key]
    return get


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("d", [4, 8, 12, 20, 36, 64, 72, 96, 100, 124, 128])
def test_relay_d_grid(amd, orc, flat_cases, monkeypatch, metric, d):
    # the three bench dimensions (relayed) and, on the one-lane-per-row form
    # every other d keeps, rows shorter than one float4 per lane of a quad
    # (d < 16) and d % 16 != 0
    k = 32
    idx, x, y = flat_cases(d, metric, 2048)
    monkeypatch.setenv("FAISS_AMD_COARSE", "bf3")
    D, I = idx.search(x, k)
    Dr, Ir = orc.knn(x, y, k, metric=metric, blas_form=True)
    assert_same_results(D, I, Dr, Ir)


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("d", [128, 96])
@pytest.mark.parametrize("k", [1, 10, 15, 16, 17, 32, 33, 64, 100])
def test_relay_k_grid(amd, orc, flat_cases, monkeypatch, metric, d, k):
    # the number of exactly evaluated rows (>= k) falls below one 16-row
    # pass, on a pass boundary and one past it, up to five passes (k = 64:
    # two 64-lane batches).  k = 100 is past kMaxK (64): IndexFlat answers it
    # on the large-k path (whole distance rows + exact select), without the
    # re-rank; the case pins that path beside the others.  The wide batches
    # are asserted in test_relay_wide_batches.
    idx, x, y = flat_cases(d, metric, 4096)
    monkeypatch.setenv("FAISS_AMD_COARSE", "bf3")
    D, I = idx.search(x, k)
    Dr, Ir = orc.knn(x, y, k, metric=metric, blas_form=True)
    assert_same_results(D, I, Dr, Ir)


def clustered(orc, d, ny, ncl, seed=43):
    """ncl rows within 1e-3 of row 0 (their thread streams overflow and are
    re-scanned exactly), 40 duplicated rows, queries near the cluster."""
    y = rand(orc, ny, d, seed)
    rng = np.random.default_rng(7)
    y[:ncl] = y[0] + 1e-3 * rng.standard_normal((ncl, d)).astype(np.float32)
    y[ny // 2: ny // 2 + 40] = y[1000:1040]
    x = np.ascontiguousarray(np.concatenate(
        [rand(orc, 150, d, seed + 1), y[:10] + np.float32(1e-3), y[1000:1010]]))
    return x, y


def parse_stats(err):
    m = re.findall(r"coarse bf3: nq=(\d+) k=(\d+) survivors/q=([\d.]+) failing streams/q=([\d.]+) "
                   r"overflow=(\d+) general-resolve=(\d+) relayed=(\d+)", err)
    assert m, f"no coarse statistics line in: {err[-400:]!r}"
    nq, k, surv, fails, over, resolve, relayed = m[-1]
    return dict(nq=int(nq), k=int(k), survivors=float(surv), fails=float(fails),
                overflow=int(over), resolve=int(resolve), relayed=int(relayed))


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("k", [10, 64])
@pytest.mark.parametrize("nsplit", [16, 0])
def test_relay_failing_streams(amd, orc, gpu, monkeypatch, metric, k, nsplit):
    # wide batches, the compaction branch and the exact_topk_resolve
    # hand-over run next to relayed queries
    d, ny = 128, 8192
    x, y = clustered(orc, d, ny, 300)
    idx = amd.IndexFlat(d, metric)
    idx.add(y)
    if nsplit:
        monkeypatch.setenv("FAISS_AMD_COARSE_NSPLIT", str(nsplit))
    monkeypatch.setenv("FAISS_AMD_COARSE", "bf3")
    D, I = idx.search(x, k)
    Dr, Ir = orc.knn(x, y, k, metric=metric, blas_form=True)
    assert_same_results(D, I, Dr, Ir)


def test_relay_beside_overflow(amd, orc, gpu, monkeypatch, capfd):
    # 1100 clustered rows cover more than two 512-row splits: the queries
    # near the cluster re-scan those splits and pass CR_CAP (512) candidates
    d, ny, k = 128, 8192, 64
    x, y = clustered(orc, d, ny, 1100)
    idx = amd.IndexFlat(d, 1)
    idx.add(y)
    monkeypatch.setenv("FAISS_AMD_COARSE_NSPLIT", "16")
    monkeypatch.setenv("FAISS_AMD_COARSE", "bf3")
    monkeypatch.setenv("FAISS_AMD_IVF_STATS", "1")
    capfd.readouterr()
    D, I = idx.search(x, k)
    st = parse_stats(capfd.readouterr().err)
    Dr, Ir = orc.knn(x, y, k, metric=1, blas_form=True)
    assert_same_results(D, I, Dr, Ir)
    assert st["overflow"] > 0 and st["relayed"] > 0


def stream_rows(slot, n):
    """The first n rows of thread stream `slot` of a split that starts at row
    0 (bf3.h ivf_stream_row: e = tile * 16 + register)."""
    return [(e >> 4) * 64 + 32 * (slot >> 1) + 4 * (slot & 1) + 8 * ((e & 15) >> 2) + (e & 3)
            for e in range(n)]


@pytest.mark.parametrize("nstreams,lo,hi", [(1, 65, 128), (2, 129, 256)])
def test_relay_wide_batches(amd, orc, gpu, monkeypatch, capfd, tmp_path, nstreams, lo, hi):
    # 16 splits of 256 rows, 64 rows per thread stream, k = 32 (KT = 8).  24
    # rows within 1e-3 of each other in each of `nstreams` streams of the first
    # split: a query beside them has 24 of its top 32 in such a stream, which
    # drops 16 of them and fails, so all its 64 rows are evaluated exactly
    # beside the other streams' survivors: 65..128 candidates with one stream
    # (two 64-lane batches), 129..256 with two (four batches).  Those queries
    # must have been relayed, with the oracle's result.
    d, ny, k = 128, 4096, 32
    y = rand(orc, ny, d, 47)
    rng = np.random.default_rng(11)
    rows = [r for s in range(nstreams) for r in stream_rows(s, 24)]
    y[rows] = y[rows[0]] + 1e-3 * rng.standard_normal((len(rows), d)).astype(np.float32)
    near = y[rows[:12]] + np.float32(1e-3)
    x = np.ascontiguousarray(np.concatenate([rand(orc, 100, d, 48), near]))
    idx = amd.IndexFlat(d, 1)
    idx.add(y)
    trace = tmp_path / "crtrace.bin"
    monkeypatch.setenv("FAISS_AMD_COARSE_NSPLIT", "16")
    monkeypatch.setenv("FAISS_AMD_COARSE", "bf3")
    monkeypatch.setenv("FAISS_AMD_IVF_STATS", "1")
    monkeypatch.setenv("FAISS_AMD_CRERANK_TRACE", str(trace))
    capfd.readouterr()
    D, I = idx.search(x, k)
    st = parse_stats(capfd.readouterr().err)
    Dr, Ir = orc.knn(x, y, k, metric=1, blas_form=True)
    assert_same_results(D, I, Dr, Ir)
    rec = np.fromfile(trace, dtype=np.uint64).reshape(-1, 8)
    ns = (rec[:, 2] & np.uint64(0xffffffff)).astype(np.int64)
    fails = (rec[:, 2] >> np.uint64(32)).astype(np.int64)
    print(f"streams {nstreams}: near queries ns {ns[100:]} failing streams {fails[100:]}; "
          f"others ns max {ns[:100].max()}; {st}")
    assert st["relayed"] == int(((ns >= 1) & (ns <= 256)).sum())
    wide = (ns[100:] >= lo) & (ns[100:] <= hi)
    assert wide.all(), "the clustered queries missed the batch range"
    # relayed queries carry the fetch stamp
    assert (rec[100:, 7] >= rec[100:, 4]).all() and (rec[100:, 7] <= rec[100:, 5]).all()


@pytest.mark.parametrize("d,k,relays", [(128, 32, True), (96, 17, True), (100, 17, False)])
def test_relay_count(amd, orc, flat_cases, monkeypatch, capfd, tmp_path, d, k, relays):
    # the relay ran: the launcher's count of relayed queries equals the number
    # of queries whose candidate count (the wave trace's word 2) is in the
    # relayed range 1..256, and that is nearly all of them.  The relay is
    # compiled for d = 64 / 96 / 128; any other d keeps one lane per row and
    # counts no relayed query.
    idx, x, y = flat_cases(d, 1, 4096)
    trace = tmp_path / "crtrace.bin"
    monkeypatch.setenv("FAISS_AMD_COARSE", "bf3")
    monkeypatch.setenv("FAISS_AMD_IVF_STATS", "1")
    monkeypatch.setenv("FAISS_AMD_CRERANK_TRACE", str(trace))
    capfd.readouterr()
    D, I = idx.search(x, k)
    st = parse_stats(capfd.readouterr().err)
    Dr, Ir = orc.knn(x, y, k, metric=1, blas_form=True)
    assert_same_results(D, I, Dr, Ir)
    rec = np.fromfile(trace, dtype=np.uint64).reshape(-1, 8)
    assert rec.shape[0] == x.shape[0] and st["nq"] == x.shape[0]
    ns = (rec[:, 2] & np.uint64(0xffffffff)).astype(np.int64)
    assert (ns >= k).all()
    expect = int(((ns >= 1) & (ns <= 256)).sum())
    print(f"relayed {st['relayed']} expected {expect} ns min/mean/max "
          f"{ns.min()}/{ns.mean():.1f}/{ns.max()}")
    assert expect >= x.shape[0] * 9 // 10
    if not relays:
        assert st["relayed"] == 0
        return
    assert st["relayed"] == expect
    # the relayed queries carry the fetch stamp between the candidate list
    # and the end of the exact evaluation
    rl = (ns >= 1) & (ns <= 256)
    assert (rec[rl, 7] >= rec[rl, 4]).all() and (rec[rl, 7] <= rec[rl, 5]).all()


def quantize_device(idx, xq, nprobe):
    """IndexIVF::quantize_device on hipMalloc'd buffers; host (dis, int32 ids)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    n = xq.shape[0]
    ptrs = []
    for nbytes in (xq.nbytes, n * nprobe * 4, n * nprobe * 4):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
        ptrs.append(p)
    px, pd, pi = ptrs
    try:
        hip.hipMemcpy(px, xq.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(xq.nbytes), 1)
        idx.quantize_device(n, px.value, nprobe, pd.value, pi.value)
        assert hip.hipDeviceSynchronize() == 0
        D = np.empty((n, nprobe), np.float32)
        I = np.empty((n, nprobe), np.int32)
        hip.hipMemcpy(D.ctypes.data_as(ctypes.c_void_p), pd, ctypes.c_size_t(D.nbytes), 2)
        hip.hipMemcpy(I.ctypes.data_as(ctypes.c_void_p), pi, ctypes.c_size_t(I.nbytes), 2)
    finally:
        for p in ptrs:
            hip.hipFree(p)
    return D, I


@pytest.mark.parametrize("out", ["int32", "int64"])
@pytest.mark.parametrize("nlist", [64, 256])
def test_relay_ivfflat_coarse(amd, orc, gpu, monkeypatch, capfd, nlist, out):
    # the IVF coarse quantizer at the bench's d / nprobe / k: int32 output
    # (quantize_device, the route the bench runs) and int64 (the quantizer's
    # search), and the IVF search.  64 lists are one 64-centroid split, which
    # has no filter plan for 32 probes (k <= 16 per split): there the f32 tile
    # answers and the case only pins the result.  256 lists have a plan, and
    # every query must have been relayed.
    d, nprobe, k = 128, 32, 10
    xb = rand(orc, 20000, d, 1234)
    idx = amd.index_factory(d, f"IVF{nlist},Flat")
    idx.train(xb)
    idx.add(xb)
    idx.nprobe = nprobe
    xq = rand(orc, 200, d, 5678)
    ref = orc.IVFOracle.from_index(idx)
    Dr, Ir = orc.knn(xq, ref.centroids, nprobe, metric=1, blas_form=True)
    monkeypatch.setenv("FAISS_AMD_IVF_STATS", "1")
    capfd.readouterr()
    if out == "int32":
        Dq, Iq = quantize_device(idx, xq, nprobe)
        Iq = Iq.astype(np.int64)
    else:
        Dq, Iq = idx.quantizer.search(xq, nprobe)
    err = capfd.readouterr().err
    assert_same_results(Dq, Iq, Dr, Ir)
    if nlist >= 128:
        st = parse_stats(err)
        print(f"nlist {nlist} {out}: {st}")
        assert st["nq"] == xq.shape[0] and st["k"] == nprobe
        assert st["overflow"] == 0 and st["relayed"] == xq.shape[0]
    else:
        assert "coarse bf3:" not in err
    monkeypatch.delenv("FAISS_AMD_IVF_STATS")
    D, I = idx.search(xq, k)
    Ds, Is, _, _ = ref.search(xq, k, nprobe, nslices=1)
    assert_same_results(D, I, Ds, Is)
