"""GPU: METRIC_INNER_PRODUCT on IndexHNSWFlat, alone and as the coarse
quantizer of IVF-Flat / IVF-PQ.

Every case of the reference-run fixtures (scripts/make_golden_hnsw_ip.py:
tests/golden/ref_hnsw_ip.npz, ref_hnsw_ip/) must come back bit-equal — D, I
and the four HNSWStats deltas.  Shapes without a fixture are held to
tests/hnsw_ip_model.py, which tests/test_hnsw_ip_model.py pins to the same
fixtures; their indexes are built by this library's host add (which
tests/test_hnsw_ip_model.py holds to the reference's bytes).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import hnsw_ip_model as im  # noqa: E402
from test_gpu_hnsw_params import make_sel, search_dev, stats  # noqa: E402
from test_gpu_coarse_relay import quantize_device  # noqa: E402

pytestmark = pytest.mark.gpu
FX = im.load_fixtures()
IP = 0  # METRIC_INNER_PRODUCT


@pytest.fixture(scope="module")
def indexes(amd, gpu):
    return {tag: amd.read_index(fn) for tag, fn in im.FILES.items()}


def params_of(amd, job):
    name, k, how, ef, chk, bnd, sel, _ = job
    return amd.SearchParametersHNSW(ef, chk, bnd, make_sel(amd, sel))


def check(amd, key, run):
    amd.cvar.hnsw_stats.reset()
    D, I = run()
    assert I.dtype == np.int64
    im.assert_case(FX, key, D, I, stats(amd))


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("tag", ["h16", "h8"])
def test_standalone_jobs_equal_reference(amd, indexes, tag):
    """The default mode at ef, k <= 64 (the register kernel), ef 200 (the
    sequential kernel) and ef 5000 / k 100 (its heaps in global scratch), the
    stop after efSearch hops and the selectors (its EXT forms), and
    bounded_queue false (k_hnsw_unbounded)."""
    idx = indexes[tag]
    xq = FX[f"{tag}_xq"]
    js = im.jobs(FX, tag)
    assert len(js) == 50
    for job in js:
        p = params_of(amd, job)
        check(amd, f"{tag}_{job[0]}", lambda: idx.search(xq, job[1], params=p))


def test_device_entry_and_search_stats(amd, indexes):
    idx = indexes["h16"]
    xq = FX["h16_xq"]
    for job in im.jobs(FX, "h16"):
        if job[3] not in (16, 200) and not job[0].startswith("sel_"):
            continue
        p = params_of(amd, job)
        check(amd, f"h16_{job[0]}", lambda: search_dev(idx, xq, job[1], p))
        check(amd, f"h16_{job[0]}", lambda: idx.search_stats(xq, job[1], p)[:2])


def test_no_fast_kernel_runs(amd, indexes):
    """Inner product is served by the sequential forms alone: the batched and
    wide kernels (and the int8 row image) never run."""
    idx = indexes["h16"]
    xq = FX["h16_xq"]
    amd.set_kernel_timing(True)
    try:
        for ef, k in ((16, 10), (64, 1), (64, 100), (200, 10), (5000, 100)):
            idx.reset_kernel_times()
            amd.cvar.hnsw_stats.reset()
            idx.efSearch = ef
            D, I = idx.search(xq, k)
            names = {nm for nm, _, _ in idx.kernel_times()}
            assert names == {"hnsw_exact"}, (ef, k, names)
            im.assert_case(FX, f"h16_def_ef{ef}_k{k}", D, I, stats(amd))
            fp32_rows, q8_rows = amd.cvar.hnsw_row_stats
            assert q8_rows == 0 and fp32_rows == stats(amd)[2]
    finally:
        amd.set_kernel_timing(False)
        idx.efSearch = 16


def test_heap_layout_form(amd, indexes, monkeypatch):
    """FAISS_AMD_HNSW_LAYOUT=1: the register kernel with faiss's heap array
    for every query instead of the sorted candidate set."""
    monkeypatch.setenv("FAISS_AMD_HNSW_LAYOUT", "1")
    for tag in ("h16", "h8"):
        for job in im.jobs(FX, tag):
            if job[0].startswith("def_") and job[3] <= 64 and job[1] <= 64:
                p = params_of(amd, job)
                check(amd, f"{tag}_{job[0]}",
                      lambda: indexes[tag].search(FX[f"{tag}_xq"], job[1], params=p))


def test_index_level_flags(amd, indexes):
    idx = indexes["h8"]
    xq = FX["h8_xq"]
    try:
        idx.efSearch = 64
        idx.check_relative_distance = False
        check(amd, "h8_A_ef64_k10", lambda: idx.search(xq, 10))
        idx.check_relative_distance, idx.search_bounded_queue = True, False
        check(amd, "h8_B_ef64_k10", lambda: idx.search(xq, 10))
        # a default-constructed params object overrides the cleared flag
        check(amd, "h8_def_ef16_k10",
              lambda: idx.search(xq, 10, params=amd.SearchParametersHNSW()))
    finally:
        idx.efSearch, idx.check_relative_distance, idx.search_bounded_queue = 16, True, True


# ---------------------------------------------------------------- IVF
@pytest.mark.parametrize("tag", ["ivfflat", "ivfpq"])
def test_ivf_quantizer_equals_reference(amd, gpu, tag):
    idx = amd.read_index(im.IVF_FILES[tag])
    q = idx.quantizer
    xq = FX[f"{tag}_xq"]
    for name, k, how, ef, chk, bnd, sel, nprobe in im.jobs(FX, tag):
        idx.nprobe = nprobe
        if how == "index":
            q.efSearch = ef
            # the quantizer on its own: the positive inner products, largest first
            Dq, Iq = q.search(xq, nprobe)
            np.testing.assert_array_equal(Iq, FX[f"{tag}_coarse_np{nprobe}_ef{ef}_I"])
            np.testing.assert_array_equal(Dq.view(np.uint32),
                                          FX[f"{tag}_coarse_np{nprobe}_ef{ef}_D"].view(np.uint32))
            # IndexIVF::quantize_device (assign_device, int32 labels): what the
            # scan and IndexShardsIVF are handed
            Dc, Ic = quantize_device(idx, xq, nprobe)
            q.fold_device_stats()  # (a device entry leaves its counters to the caller)
            assert Ic.dtype == np.int32
            np.testing.assert_array_equal(Ic, FX[f"{tag}_coarse_np{nprobe}_ef{ef}_I"])
            np.testing.assert_array_equal(Dc.view(np.uint32),
                                          FX[f"{tag}_coarse_np{nprobe}_ef{ef}_D"].view(np.uint32))
            check(amd, f"{tag}_{name}", lambda: idx.search(xq, k))
            check(amd, f"{tag}_{name}", lambda: search_dev(idx, xq, k, None))
            # search_preassigned fed the reference's coarse output
            D, I = idx.search_preassigned(xq, k, FX[f"{tag}_coarse_np{nprobe}_ef{ef}_I"],
                                          FX[f"{tag}_coarse_np{nprobe}_ef{ef}_D"])
            im.assert_case(FX, f"{tag}_{name}", D, I)
        else:
            q.efSearch = 16
            sp = amd.SearchParametersIVF(
                nprobe=nprobe, quantizer_params=amd.SearchParametersHNSW(ef, chk, bnd))
            check(amd, f"{tag}_{name}", lambda: idx.search(xq, k, params=sp))
            check(amd, f"{tag}_{name}", lambda: search_dev(idx, xq, k, sp))


def test_ivf_search_captured_graph_replay_equals_eager(amd, gpu):
    """search_device of an inner-product IVF64_HNSW8,Flat captured with
    torch.cuda.graph (IndexIVF's own search graph takes flat quantizers only)
    and replayed: on the captured queries and on other queries written into
    the same buffer, the eager results bit for bit.  The path has no host
    read-back (no split: hnsw_uses_batched is false) and, after the warm-up,
    no allocation."""
    import torch
    idx = amd.read_index(im.IVF_FILES["ivfflat"])
    idx.nprobe = 8
    idx.quantizer.efSearch = 64
    xq = np.ascontiguousarray(FX["ivfflat_xq"], dtype=np.float32)
    n, k = xq.shape[0], 10
    x_t = torch.from_numpy(xq).cuda()
    D_t = torch.empty((n, k), dtype=torch.float32, device="cuda")
    I_t = torch.empty((n, k), dtype=torch.int64, device="cuda")
    ts = torch.cuda.Stream()

    def call():
        idx.search_device(n, x_t.data_ptr(), k, D_t.data_ptr(), I_t.data_ptr(), ts.cuda_stream)

    def eager(x):
        x_t.copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        call()
        ts.synchronize()
        return D_t.cpu().numpy().copy(), I_t.cpu().numpy().copy()

    xq2 = np.ascontiguousarray(xq[::-1])
    ref2 = eager(xq2)
    ref = eager(xq)  # (also the warm-up: every scratch buffer has its size)
    eager(xq)
    im.assert_case(FX, "ivfflat_np8_ef64", ref[0], ref[1])
    np.testing.assert_array_equal(ref2[1], ref[1][::-1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=ts):
        call()
    for x, want in ((xq, ref), (xq2, ref2), (xq, ref)):
        x_t.copy_(torch.from_numpy(x))
        D_t.zero_()
        I_t.fill_(-7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(I_t.cpu().numpy(), want[1])
        np.testing.assert_array_equal(D_t.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


# ---------------------------------------------------------------- model shapes
MODES = [("def", dict()), ("A", dict(check_relative_distance=False)),
         ("B", dict(bounded_queue=False)), ("sel", dict()),
         ("selA", dict(check_relative_distance=False))]


def vs_model(amd, orc, idx, xq, k, ef, modes=MODES, device=True, member=None, counters=True):
    m = im.Model(orc, orc.HNSWGraph.from_index(idx))
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
            np.testing.assert_array_equal(D.view(np.uint32), Dm.view(np.uint32), err_msg=name)
            assert not counters or stats(amd) == [int(v) for v in stm], name
    return m


def scaled_rows(orc, n, d, seed):
    """Signed rows of very different lengths (the largest inner product is
    then not the nearest row)."""
    x = orc.float_rand(n * d, seed).reshape(n, d) - np.float32(0.5)
    s = np.float32(0.25) + np.float32(3.75) * orc.float_rand(n, seed + 1)
    return np.ascontiguousarray(x * s[:, None], dtype=np.float32)


@pytest.mark.parametrize("M", [4, 32])
@pytest.mark.parametrize("d", [4, 8, 20, 100, 132])
def test_dimensions_equal_model(amd, orc, gpu, d, M):
    """d = 4, 20, 100, 132: ref_ip's 4-term epilogue; d = 8: none; d = 132:
    past the 4-lanes-per-row form (a second LDS trip of the query); 3000 rows
    with duplicates; ef, k <= 64 (register kernel) and k > ef > 64."""
    idx = amd.IndexHNSWFlat(d, M, IP)
    xb = scaled_rows(orc, 3000, d, 900 + d)
    xb[2900:] = xb[:100]
    idx.add(xb)
    xq = np.concatenate([scaled_rows(orc, 6, d, 901 + d), xb[:2]])
    for ef, k in ((8, 3), (40, 70)):
        vs_model(amd, orc, idx, xq, k, ef)


def test_fma_tail_equals_model(amd, orc, gpu):
    """d = 13 (ld 16): the 4-term epilogue and one fma-tail term; host search
    only (the device entry needs d % 4 == 0)."""
    idx = amd.IndexHNSWFlat(13, 8, IP)
    xb = scaled_rows(orc, 500, 13, 77)
    idx.add(xb)
    xq = np.concatenate([scaled_rows(orc, 6, 13, 78), xb[:2]])
    for ef, k in ((8, 3), (40, 70)):
        vs_model(amd, orc, idx, xq, k, ef, device=False)


@pytest.mark.parametrize("M", [4, 32])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_small_indexes_equal_model(amd, orc, gpu, n, M):
    """ntotal around the wave size, k below and above ntotal (padding)."""
    idx = amd.IndexHNSWFlat(8, M, IP)
    xb = scaled_rows(orc, n, 8, 300 + n)
    idx.add(xb)
    xq = np.concatenate([scaled_rows(orc, 5, 8, 301 + n), xb[:1]])
    for ef, k in ((4, 1), (16, 70)):
        vs_model(amd, orc, idx, xq, k, ef)


def test_empty_index(amd, orc, gpu):
    idx = amd.IndexHNSWFlat(8, 8, IP)
    xq = scaled_rows(orc, 5, 8, 3)
    for kw in (dict(), dict(check_relative_distance=False), dict(bounded_queue=False),
               dict(sel=amd.IDSelectorRange(0, 4))):
        amd.cvar.hnsw_stats.reset()
        D, I = idx.search(xq, 3, params=amd.SearchParametersHNSW(4, **kw))
        assert (I == -1).all() and (D == -im.FLT_MAX).all() and stats(amd) == [0, 0, 0, 0]


def test_visited_bitmap_in_global_scratch(amd, orc, gpu):
    """640,000 nodes: the visited bitmap (80 KB per query) no longer fits the
    LDS and lives in global scratch, for every kernel form."""
    d, n = 4, 640_000
    idx = amd.IndexHNSWFlat(d, 4, IP)
    idx.efConstruction = 8
    idx.add(scaled_rows(orc, n, d, 11))
    xq = scaled_rows(orc, 6, d, 12)
    for ef, k in ((16, 5), (100, 70)):
        vs_model(amd, orc, idx, xq, k, ef, modes=MODES[:3])


def test_zero_and_nan_queries_equal_model(amd, orc, gpu):
    """An all-zero query (every distance -0.0: ties everywhere), counters
    included.  A query with a NaN component (every distance NaN): ids and
    distances — no distance is ever below the result threshold, so every slot
    is padding.  Its HNSWStats are left out: every comparison of the
    reference's heaps is then false and its traversal follows the accidents
    of its heap array, while the kernels order their 64-bit keys with NaN
    above FLT_MAX (for both metrics)."""
    idx = amd.IndexHNSWFlat(8, 8, IP)
    xb = scaled_rows(orc, 500, 8, 21)
    idx.add(xb)
    xq = scaled_rows(orc, 4, 8, 22)
    xq[1] = 0
    xn = scaled_rows(orc, 3, 8, 23)
    xn[1, 3] = np.nan
    for ef, k in ((8, 3), (40, 70)):
        vs_model(amd, orc, idx, xq, k, ef)
        bounded = [m for m in MODES if m[0] != "B"]  # (B has no result threshold to hold NaN to)
        vs_model(amd, orc, idx, xn[1:2], k, ef, modes=bounded, counters=False)
        D, I = idx.search(xn, k, params=amd.SearchParametersHNSW(ef))
        assert (I[1] == -1).all() and (D[1] == -im.FLT_MAX).all()
        Dm, Im, _ = im.Model(orc, orc.HNSWGraph.from_index(idx)).search(xn[[0, 2]], k, ef)
        np.testing.assert_array_equal(I[[0, 2]], Im)  # (its neighbours in the batch: unharmed)
        np.testing.assert_array_equal(D[[0, 2]].view(np.uint32), Dm.view(np.uint32))


# ---------------------------------------------------------------- drop-in
def _compile(tmp_path, name):
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "hnsw-ivf_amd", "lib")
    exe = str(tmp_path / name)
    src = os.path.join(HERE, "c", name)
    if name.endswith(".c"):
        cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{inc}", src,
               "-o", exe, f"-L{libdir}", "-lfaiss_amd", f"-Wl,-rpath,{libdir}"]
    else:
        cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
               "-I/opt/rocm/include", f"-I{inc}", src, "-o", exe, f"-L{libdir}", "-lfaiss_amd",
               f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True)
    return exe


def test_c_and_cpp_consumers(amd, orc, gpu, tmp_path):
    """The C API (faiss_amd_IndexHNSWFlat_new_with, faiss_index_factory) and
    faiss::IndexHNSWFlat(d, M, faiss::METRIC_INNER_PRODUCT) on the rows of
    hnsw8_ip_d16: the graph they build is the reference's, so the results
    are the fixture's."""
    xb = orc.idx_storage(amd.read_index(im.FILES["h8"]))
    xq = FX["h8_xq"]
    nb, d = xb.shape
    xb.astype(np.float32).tofile(tmp_path / "xb.f32")
    xq.astype(np.float32).tofile(tmp_path / "xq.f32")
    common = [str(d), "8", str(nb), str(tmp_path / "xb.f32"), str(len(xq)),
              str(tmp_path / "xq.f32"), "64", "10"]
    c, cpp = _compile(tmp_path, "hnsw_ip.c"), _compile(tmp_path, "hnsw_ip.cpp")
    for i, cmd in enumerate(([c, "new"], [c, "factory"], [cpp])):
        out = str(tmp_path / f"o{i}.bin")
        r = subprocess.run(cmd + common + [out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        raw = np.fromfile(out, dtype=np.uint8)
        D = raw[:len(xq) * 40].view(np.float32).reshape(len(xq), 10)
        I = raw[len(xq) * 40:].view(np.int64).reshape(len(xq), 10)
        im.assert_case(FX, "h8_def_ef64_k10", D, I)
