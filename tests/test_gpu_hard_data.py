"""Every certified filter path against the oracle on the distributions of
tests/hard_data.py, bit for bit (ids and distances): signed values, offsets
that put every candidate inside the margin window and make L2 approximations
non-positive, one dominant coordinate, near-ties under a margin of ~1e3, zero
rows and queries, and non-finite rows and queries.  2048 rows, 8 lists whose
centroids are 8 database rows (no k-means between the data and the
comparison), 64 queries, nprobe 4.

Also here: the audit of the IVF-Flat filter's own brackets from its key dump
(FAISS_AMD_IVF_DUMP) against float64 distances, and the power-of-two scaling
identity (scaling every input by 2^s scales the distances by 2^2s exactly).
test_bf16_margin_model.py holds the numpy restatement of the same margins.
"""
import numpy as np
import pytest

import hard_data
from conftest import assert_same_results
from pq_nbits_model import Model
from test_gpu_refine import composed
from test_ref_hard_fixtures import IN, path, xq_of

pytestmark = pytest.mark.gpu

NB, NQ, NLIST, NPROBE, SEED = 2048, 64, 8, 4, 9000
DISTS = hard_data.FINITE
CENT_ROWS = [3, 260, 517, 774, 1031, 1288, 1545, 1802]  # 8 rows, 8 different `tight` centres


def dataset(dist, d):
    xb = hard_data.make(dist, NB, d, SEED + d)
    return xb, hard_data.queries(dist, xb, NQ, SEED + d)


def stages(amd, idx, fn):
    amd.set_kernel_timing(True)
    try:
        idx.reset_kernel_times()
        out = fn()
        names = {nm for nm, _, _ in idx.kernel_times()}
    finally:
        amd.set_kernel_timing(False)
    return out, names


def build_ivf_flat(amd, xb, metric, add=True):
    d = xb.shape[1]
    quant = amd.IndexFlat(d, metric)
    quant.add(np.ascontiguousarray(xb[CENT_ROWS]))
    idx = amd.IndexIVFFlat(quant, d, NLIST, metric)
    if add:
        idx.add(xb)
    idx.nprobe = NPROBE
    return idx


# ------------------------------------------------------------------ IVF-Flat
# (scan, filter, precision, fold): the streamed bf16x2 filter with and without
# the fold image, the staged kernel, bf16x3, and the exact scan
FLAT_PATHS = [("mfma", None, None, "1"), ("mfma", None, None, "0"), ("mfma", "staged", None, "1"),
              ("mfma", None, "bf16x3", "1"), ("exact", None, None, "1")]


def run_flat_paths(amd, orc, make_index, xq, ks, capfd, want_failing=False):
    ref = None
    for scan, filt, prec, fold in FLAT_PATHS:
        mp = pytest.MonkeyPatch()
        try:
            mp.setenv("FAISS_AMD_IVF_SCAN", scan)
            mp.setenv("FAISS_AMD_IVF_FOLD", fold)   # read when the index is uploaded
            mp.setenv("FAISS_AMD_IVF_STATS", "1")
            if filt:
                mp.setenv("FAISS_AMD_IVF_FILTER", filt)
            if prec:
                mp.setenv("FAISS_AMD_IVF_PREC", prec)
            idx = make_index()
            idx.nprobe = NPROBE
            if ref is None:
                o = orc.IVFOracle.from_index(idx)
                ref = {k: o.search(xq, k, NPROBE, nslices=1)[:2] for k in ks}
            for k in ks:
                capfd.readouterr()
                (D, I), names = stages(amd, idx, lambda: idx.search(xq, k))
                err = capfd.readouterr().err
                assert_same_results(D, I, *ref[k])
                if scan == "mfma" and k <= 32:   # the filter serves k <= 32 (ivf_mfma_kq)
                    assert "ivf_flat_scan" in names and "ivf mfma scan" in err, (names, err)
                    if want_failing:
                        fp = float(err.split("failing probes/q=")[1].split()[0])
                        with capfd.disabled():
                            print(f"{scan} {filt} {prec} fold={fold} k={k}: failing probes/q={fp}")
                        assert fp > 0, err
                else:
                    assert "ivf_exact_scan" in names and "ivf_flat_scan" not in names, names
        finally:
            mp.undo()


@pytest.mark.parametrize("d", [64, 36])
@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("dist", DISTS)
def test_ivf_flat_paths_equal_oracle(amd, orc, gpu, capfd, dist, metric, d):
    xb, xq = dataset(dist, d)
    # offset4: every candidate is inside the window; k = 32 is the largest the
    # filter serves (more than 256 candidates per query), k = 64 the exact scan
    ks = (1, 10, 32, 64) if dist == "offset4" else (1, 10)
    run_flat_paths(amd, orc, lambda: build_ivf_flat(amd, xb, metric), xq, ks, capfd,
                   want_failing=dist == "offset4" and metric == 1)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivf_flat_paths_nonfinite(amd, orc, gpu, capfd, metric):
    """the reference-written index whose lists hold rows with NaN, +-inf and
    FLT_MAX coordinates; queries 5 and 6 carry a NaN and a +inf coordinate"""
    tag = f"flat_{metric}_nonfinite"
    run_flat_paths(amd, orc, lambda: amd.read_index(path(tag)), xq_of(tag), (1, 10), capfd)


# ------------------------------------------------------------------ IndexFlat
COARSE_PATHS = [{}, {"FAISS_AMD_COARSE_PREC": "bf16x2"}, {"FAISS_AMD_COARSE_FOLD": "0"},
                {"FAISS_AMD_COARSE_NSPLIT": "16"}, {"FAISS_AMD_COARSE": "f32"}]


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("dist", hard_data.NAMES)
def test_index_flat_paths_equal_oracle(amd, orc, gpu, monkeypatch, dist, metric):
    """the coarse bf16x3 stream + k_coarse_rerank (the default), its bf16x2
    alternate, the unfolded image, 16 splits, and the f32 tile"""
    xb, xq = dataset(dist, 64)
    ref = {k: orc.knn(xq, xb, k, metric=metric, blas_form=True) for k in (1, 10, 64)}
    for env in COARSE_PATHS:
        monkeypatch.setenv("FAISS_AMD_COARSE", "bf3")
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        idx = amd.IndexFlat(64, metric)   # FAISS_AMD_COARSE_FOLD is read at upload
        idx.add(xb)
        for k in (1, 10, 64):
            D, I = idx.search(xq, k)
            assert_same_results(D, I, *ref[k])
        for name in env:
            monkeypatch.delenv(name)


# ------------------------------------------------------------------ IVF-PQ
@pytest.mark.parametrize("dist", ["signed", "offset4", "heavy"])
def test_ivfpq8_filter_equals_oracle(amd, orc, gpu, dist):
    """k_ivfpq_filter_w on the reference-trained codebook of the same data"""
    idx = amd.read_index(path(f"pq8_{dist}"))
    idx.nprobe = NPROBE
    xq = IN[f"{dist}_d64_xq"]
    ref = orc.IVFOracle.from_index(idx)
    for table in (1, 0):
        idx.use_precomputed_table = table
        ref.use_precomputed_table = table
        for k in (1, 10):
            (D, I), names = stages(amd, idx, lambda: idx.search(xq, k))
            assert "ivfpq_filter" in names, names
            assert_same_results(D, I, *ref.search(xq, k, NPROBE, nslices=1)[:2])


@pytest.mark.parametrize("dist", ["signed", "offset4", "heavy"])
def test_ivfpq8_inner_product_equals_oracle(amd, orc, gpu, dist):
    xb, xq = dataset(dist, 64)
    quant = amd.IndexFlat(64, 0)
    quant.add(np.ascontiguousarray(xb[CENT_ROWS]))
    idx = amd.IndexIVFPQ(quant, 64, NLIST, 16, 8, 0)
    idx.train(xb)
    idx.add(xb)
    idx.nprobe = NPROBE
    ref = orc.IVFOracle.from_index(idx)
    for k in (1, 10):
        D, I = idx.search(xq, k)
        assert_same_results(D, I, *ref.search(xq, k, NPROBE, nslices=1)[:2])


@pytest.mark.parametrize("dist", ["signed", "offset4", "heavy"])
def test_ivfpq4_lds_table_scan_equals_model(amd, gpu, dist):
    idx = amd.read_index(path(f"pq4_{dist}"))
    idx.nprobe = NPROBE
    xq = IN[f"{dist}_d64_xq"]
    Dq, Iq = idx.quantizer.search(xq, NPROBE)
    for table in (1, 0):
        idx.use_precomputed_table = table
        m = Model.from_index(idx, table=table)
        for k in (1, 10):
            D, I = idx.search(xq, k)
            assert_same_results(D, I, *m.search_preassigned(xq, k, Iq, Dq))


# ------------------------------------------------------------------ HNSW
@pytest.fixture(scope="module")
def hnsw_heavy(amd, gpu):
    xb, xq = dataset("heavy", 64)
    idx = amd.index_factory(64, "HNSW16,Flat")
    idx.add(xb)
    return idx, xq


@pytest.mark.parametrize("q8", ["1", "0"])
@pytest.mark.parametrize("dist", ["signed", "offset100", "tight", "heavy"])
def test_hnsw_equals_oracle(amd, orc, gpu, monkeypatch, hnsw_heavy, dist, q8):
    """the int8 prefilter's lower bound under cancellation (offset100), a
    dominant coordinate and near-ties; graphs as the reference wrote them"""
    monkeypatch.setenv("FAISS_AMD_HNSW_Q8", q8)
    if dist == "heavy":
        idx, xq = hnsw_heavy
    else:
        idx, xq = amd.read_index(path(f"hnsw_{dist}")), IN[f"{dist}_d64_xq"]
    g = orc.HNSWGraph.from_index(idx)
    for ef in (16, 64):
        idx.efSearch = ef
        D, I = idx.search(xq, 10)
        assert_same_results(D, I, *g.search(xq, 10, ef))


# ------------------------------------------------------------------ RFlat
@pytest.mark.parametrize("dist", ["offset4", "tight"])
def test_refine_flat_equals_composition(amd, orc, gpu, dist):
    xb, xq = dataset(dist, 64)
    base = build_ivf_flat(amd, xb, 1, add=False)
    idx = amd.IndexRefineFlat(base)
    idx.add(xb)
    idx.k_factor = 4
    _, Ib = base.search(xq, 40)
    D, I = idx.search(xq, 10)
    assert_same_results(D, I, *composed(orc, xq, xb, Ib, 10, True))


# ------------------------------------------------------------------ the filter's own brackets
def ivf_bf3_obits(max_list_len):  # kernels_ivf_mfma.hip ivf_bf3_obits
    tiles = max(1, (max_list_len + 63) // 64)
    b = 0
    while (1 << b) < tiles:
        b += 1
    return 4 + b


def key_rows(ordv, slot):  # bf3.h ivf_key_row / ivf_stream_row
    r = ordv & 15
    return (ordv >> 4) * 64 + 32 * (slot >> 1) + 4 * (slot & 1) + 8 * (r >> 2) + (r & 3)


def decode(key, mask, l2, fold):  # bf3.h key_decode_lo/hi, fold_decode_lo/hi
    lo, hi = key & ~np.uint32(mask), key | np.uint32(mask)
    if fold:
        return (np.maximum(np.float32(-2) * lo.view(np.float32), np.float32(0)),
                np.maximum(np.float32(-2) * hi.view(np.float32), np.float32(0)))
    if l2:
        return lo.view(np.float32), hi.view(np.float32)

    def un(u):
        return (u ^ (~(u.view(np.int32) >> 31).view(np.uint32) | np.uint32(0x80000000))).view(
            np.float32)
    return un(lo), un(hi)


AUDIT_PATHS = [("stream", "1", None), ("stream", "0", None), ("staged", "1", None),
               ("staged", "1", "bf16x3")]
RATIOS = {}


def audit(amd, xb, xq, metric, filt, fold_env, prec, k, tmp_path):
    """Runs one search_preassigned with the dump on; checks every kept key's
    bracket and every stream's dropped bound against float64 distances.
    Returns the largest |approx_mid - exact| / mmax."""
    d, l2 = xb.shape[1], metric == 1
    dump = str(tmp_path / "keys.bin")
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("FAISS_AMD_IVF_SCAN", "mfma")
        mp.setenv("FAISS_AMD_IVF_FOLD", fold_env)
        mp.setenv("FAISS_AMD_GRAPH", "0")  # the dump synchronises its stream: no graph capture
        if filt == "staged":
            mp.setenv("FAISS_AMD_IVF_FILTER", "staged")
        if prec:
            mp.setenv("FAISS_AMD_IVF_PREC", prec)
        idx = build_ivf_flat(amd, xb, metric)
        Dq, Iq = idx.quantizer.search(xq, NPROBE)
        mp.setenv("FAISS_AMD_IVF_DUMP", dump)
        idx.search_preassigned(xq, k, Iq, Dq)
        mp.delenv("FAISS_AMD_IVF_DUMP")
    finally:
        mp.undo()
    n, npb = xq.shape[0], NPROBE
    DB = (d + 31) // 32 * 32
    raw = np.fromfile(dump, np.uint8)
    KE = (raw.size - n * npb * 32 - 4 * (2 * DB + 16)) // (4 * n * npb)
    assert KE in (8, 16, 32) and raw.size == n * npb * (4 * KE + 32) + 4 * (2 * DB + 16)
    KT = KE // 4
    keys = raw[:4 * n * npb * KE].view(np.uint32).reshape(n, npb, 4, KT)
    recs = raw[4 * n * npb * KE:][:32 * n * npb].view(np.uint32).reshape(n, npb, 8)
    pb, mmax = recs[..., :4].view(np.float32), recs[..., 4].view(np.float32)
    sizes = [idx.get_list_size(l) for l in range(NLIST)]
    mask = (1 << ivf_bf3_obits(max(sizes))) - 1
    fold = l2 and filt == "stream" and fold_env == "1"
    lists = [xb[idx.list_ids(l)].astype(np.float64) for l in range(NLIST)]
    worst, nkept, nbound = 0.0, 0, 0
    for q in range(n):
        x = xq[q].astype(np.float64)
        for p in range(npb):
            l = int(Iq[q, p])
            if l < 0 or sizes[l] == 0:   # no work item: the record is the empty one
                assert (keys[q, p] == 0xffffffff).all() and np.isinf(pb[q, p]).all()
                continue
            ln = sizes[l]
            assert recs[q, p, 6] == ln
            y = lists[l]
            exact = ((y - x) ** 2).sum(1) if l2 else -(y @ x)
            m = float(mmax[q, p])
            assert np.isfinite(m) and m > 0
            for sl in range(4):
                kk = keys[q, p, sl]
                kk = kk[kk != 0xffffffff]
                rows = key_rows(kk & np.uint32(mask), sl).astype(np.int64)
                # padding rows are never kept
                assert (rows < ln).all(), (q, p, sl, rows, ln)
                assert np.unique(rows).size == rows.size
                lo, hi = decode(kk, mask, l2, fold)
                ex = exact[rows]
                assert (lo.astype(np.float64) - m <= ex).all(), (q, p, sl)
                assert (ex <= hi.astype(np.float64) + m).all(), (q, p, sl)
                mid = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
                if rows.size:
                    worst = max(worst, float((np.abs(mid - ex) / m).max()))
                nkept += rows.size
                if np.isfinite(pb[q, p, sl]):
                    e = np.arange(((ln + 63) // 64) * 16)
                    srows = key_rows(e, sl)
                    dropped = np.setdiff1d(srows[srows < ln], rows)
                    assert (exact[dropped] >= float(pb[q, p, sl])).all(), (q, p, sl)
                    nbound += 1
    assert nkept > 0 and nbound > 0
    return worst


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("dist", ["uniform", "offset1", "offset100", "heavy", "tight", "signed"])
def test_filter_brackets_hold_against_float64(amd, gpu, tmp_path, dist, metric):
    """decode_lo - mmax <= exact <= decode_hi + mmax for every kept key, and
    every row a stream dropped has exact >= its dropped bound; staged and
    streamed kernel, plain and folded keys, bf16x2 and bf16x3.  The only
    threshold is 1: the recorded ratios are printed, not asserted."""
    xb, xq = dataset(dist, 64)
    for filt, fold_env, prec in AUDIT_PATHS:
        if metric == 0 and fold_env == "0":
            continue  # inner product has no fold image: same kernel as fold=1
        r = max(audit(amd, xb, xq, metric, filt, fold_env, prec, k, tmp_path) for k in (1, 10))
        RATIOS[(dist, metric, filt, fold_env, prec)] = r
        print(f"audit {dist} {'L2' if metric else 'IP'} {filt} fold={fold_env} "
              f"{prec or 'bf16x2'}: max |mid - exact| / mmax = {r:.3f}")
        assert r <= 1.0


# ------------------------------------------------------------------ power-of-two scaling
SCALES = [40, -40]


def scaled_equal(D, I, Ds, Is, s):
    np.testing.assert_array_equal(Is, I)
    np.testing.assert_array_equal(Ds, D * np.float32(2.0 ** (2 * s)))


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("dist", ["signed", "offset4", "heavy", "tight", "sparse"])
def test_scaling_ivf_flat_and_index_flat(amd, gpu, dist, metric, s):
    """an absolute constant (1e-30f, 1e-38f) or a threshold that is not
    scale-free may widen a margin, never change a result"""
    xb, xq = dataset(dist, 64)
    xbs, xqs = hard_data.pow2(xb, s), hard_data.pow2(xq, s)
    a, b = build_ivf_flat(amd, xb, metric), build_ivf_flat(amd, xbs, metric)
    for k in (1, 10):
        scaled_equal(*a.search(xq, k), *b.search(xqs, k), s)
    fa, fb = amd.IndexFlat(64, metric), amd.IndexFlat(64, metric)
    fa.add(xb)
    fb.add(xbs)
    for k in (1, 10):
        scaled_equal(*fa.search(xq, k), *fb.search(xqs, k), s)


def scaled_copy(amd, idx, arrays, s, tmp_path):
    """idx with the given float arrays (found once each in its file image)
    multiplied by 2^s: the same lists, codes and graph over scaled vectors"""
    a, b = str(tmp_path / "a.faiss"), str(tmp_path / "b.faiss")
    amd.write_index(idx, a)
    with open(a, "rb") as f:
        blob = f.read()
    for arr in arrays:
        old = np.ascontiguousarray(arr, np.float32).tobytes()
        assert blob.count(old) == 1
        blob = blob.replace(old, hard_data.pow2(arr, s).tobytes())
    with open(b, "wb") as f:
        f.write(blob)
    return amd.read_index(b)


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("dist", ["signed", "offset4", "heavy"])
def test_scaling_ivfpq8(amd, gpu, tmp_path, dist, s):
    """coarse centroids, PQ codebook and queries scaled; the codes stay"""
    idx = amd.read_index(path(f"pq8_{dist}"))
    sc = scaled_copy(amd, idx, [idx.quantizer.xb, idx.pq_centroids], s, tmp_path)
    xq = IN[f"{dist}_d64_xq"]
    idx.nprobe = sc.nprobe = NPROBE
    for table in (1, 0):
        idx.use_precomputed_table = sc.use_precomputed_table = table
        for k in (1, 10):
            scaled_equal(*idx.search(xq, k), *sc.search(hard_data.pow2(xq, s), k), s)


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("dist", ["signed", "offset100", "tight"])
def test_scaling_hnsw(amd, gpu, tmp_path, dist, s):
    idx = amd.read_index(path(f"hnsw_{dist}"))
    sc = scaled_copy(amd, idx, [idx.storage_vectors()], s, tmp_path)
    xq = IN[f"{dist}_d64_xq"]
    for ef in (16, 64):
        idx.efSearch = sc.efSearch = ef
        scaled_equal(*idx.search(xq, 10), *sc.search(hard_data.pow2(xq, s), 10), s)
