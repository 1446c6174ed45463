"""CPU checks against the reference-run fixtures on hard data
(tests/golden/ref_hard*, oracle/ref/make_golden_hard.py): IVF-Flat, IVF-PQ,
IVF-SQ and HNSW indexes the reference built over the distributions of
tests/hard_data.py (signed, offset, one dominant coordinate, near-ties, zero
rows, non-finite rows) and the results of its own searches over them.

  * the inputs are pinned: hard_data regenerates the stored queries and the
    database whose rows the flat index files hold;
  * the product's reader parses every file and writes it back byte for byte;
  * the oracle restatement reproduces every reference output bit for bit:
    search_preassigned on the reference's own probes everywhere, the coarse
    quantizer (BLAS form) and the end-to-end search where MKL's sgemm and the
    oracle's k-ordered fma chain agree (see COARSE_DIFFERS);
  * multiplying every input by 2^s (s = +40, -40) multiplies the oracle's
    distances by 2^2s exactly and leaves the ids alone.
The GPU path is checked against the same arrays in test_gpu_hard_fixtures.py.
"""
import hashlib
import os

import numpy as np
import pytest

import hard_data
from pq_nbits_model import Model

HERE = os.path.dirname(os.path.abspath(__file__))
GDIR = os.path.join(HERE, "golden", "ref_hard")
IN = np.load(os.path.join(HERE, "golden", "ref_hard.npz"))
NB, NQ, SEED = 2048, 64, 9000

L2_DISTS = ["signed", "offset1", "offset4", "offset100", "heavy", "tight", "sparse", "nonfinite"]
IP_DISTS = ["signed", "sparse", "heavy", "nonfinite"]
PQ_DISTS = ["signed", "offset4", "heavy"]
HNSW_DISTS = ["signed", "offset100", "tight"]
FLAT_TAGS = ([f"flat_l2_{x}" for x in L2_DISTS] + [f"flat_ip_{x}" for x in IP_DISTS] +
             ["flat_l2_d36_offset4"])
PQ8_TAGS = [f"pq8_{x}" for x in PQ_DISTS]
PQ4_TAGS = [f"pq4_{x}" for x in PQ_DISTS]
HNSW_TAGS = [f"hnsw_{x}" for x in HNSW_DISTS]
SQ_TAGS = ["sq8_signed", "sq8_offset4", "sqfp16_signed", "sqfp16_offset4"]
ALL_TAGS = FLAT_TAGS + PQ8_TAGS + PQ4_TAGS + SQ_TAGS + HNSW_TAGS


def path(tag):
    return os.path.join(GDIR, tag + ".faiss")


def results(tag):
    return np.load(os.path.join(GDIR, tag + ".npz"))


def dist_d(tag):
    return tag.rsplit("_", 1)[1], 36 if "_d36_" in tag else 64


def xq_of(tag):
    dist, d = dist_d(tag)
    return IN[f"{dist}_d{d}_xq"]


def pre_cases(fx):
    """(key, table or None, nprobe, k) of every search_preassigned record"""
    for key in fx.files:
        if "pre_" not in key or not key.endswith("_D"):
            continue
        parts = key[:-2].split("_")
        table = int(parts[0][1:]) if parts[0].startswith("t") else None
        yield key[:-2], table, int(parts[-2]), int(parts[-1])


def test_only_index_files_and_arrays():
    names = sorted(os.listdir(GDIR))
    assert sorted(t + e for t in ALL_TAGS for e in (".faiss", ".npz")) == names
    for n in names:
        assert os.path.getsize(os.path.join(GDIR, n)) < (1 << 20), n


@pytest.mark.parametrize("dist,d", [(x, 64) for x in L2_DISTS] + [("offset4", 36)])
def test_inputs_are_the_named_distributions(amd, dist, d):
    xb = hard_data.make(dist, NB, d, SEED + d)
    sha = np.frombuffer(hashlib.sha256(xb.tobytes()).digest(), np.uint8)
    np.testing.assert_array_equal(sha, IN[f"{dist}_d{d}_xb_sha"])
    np.testing.assert_array_equal(hard_data.queries(dist, xb, NQ, SEED + d).view(np.uint32),
                                  IN[f"{dist}_d{d}_xq"].view(np.uint32))
    idx = amd.read_index(path(f"flat_l2_{dist}" if d == 64 else "flat_l2_d36_offset4"))
    _, codes, ids = idx.invlists_arrays()
    got = np.empty((NB, d), np.float32)
    got[ids] = codes.view(np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), xb.view(np.uint32))


def test_nonfinite_rows_sit_where_the_filters_can_go_wrong(amd):
    """several lists, different 64-row tiles, one the first row of its list"""
    idx = amd.read_index(path("flat_l2_nonfinite"))
    where = {}
    for l in range(idx.nlist):
        ids = idx.list_ids(l)
        for r, _, _ in hard_data.NONFINITE_ROWS:
            pos = np.nonzero(ids == r)[0]
            if pos.size:
                where[r] = (l, int(pos[0]))
    assert len(where) == len(hard_data.NONFINITE_ROWS)
    assert len({l for l, _ in where.values()}) >= 2
    assert len({p // 64 for _, p in where.values()}) >= 3
    assert where[0][1] == 0


@pytest.mark.parametrize("tag", ALL_TAGS)
def test_rewrite_reference_file_byte_identical(amd, tag, tmp_path):
    idx = amd.read_index(path(tag))
    assert idx.ntotal == NB
    out = str(tmp_path / "re.faiss")
    amd.write_index(idx, out)
    with open(path(tag), "rb") as f1, open(out, "rb") as f2:
        assert f1.read() == f2.read()


@pytest.mark.parametrize("tag", FLAT_TAGS + PQ8_TAGS)
def test_oracle_preassigned_equals_reference(amd, orc, tag):
    idx = amd.read_index(path(tag))
    ref = orc.IVFOracle.from_index(idx)
    fx, xq = results(tag), xq_of(tag)
    n = 0
    for key, table, nprobe, k in pre_cases(fx):
        if table is not None:
            ref.use_precomputed_table = table
        D, I = ref.search_preassigned(xq, k, fx[f"q{nprobe}_I"], fx[f"q{nprobe}_D"])
        np.testing.assert_array_equal(I, fx[key + "_I"], err_msg=key)
        np.testing.assert_array_equal(D, fx[key + "_D"], err_msg=key)
        n += 1
    assert n == (12 if tag in PQ8_TAGS else 6)


@pytest.mark.parametrize("tag", PQ4_TAGS)
def test_model_pq4_preassigned_equals_reference(amd, tag):
    """4-bit codes: the numpy model of tests/pq_nbits_model.py"""
    idx = amd.read_index(path(tag))
    fx, xq = results(tag), xq_of(tag)
    for table in (1, 0):
        m = Model.from_index(idx, table=table)
        for nprobe, k in ((4, 10), (8, 100)):
            D, I = m.search_preassigned(xq, k, fx[f"q{nprobe}_I"], fx[f"q{nprobe}_D"])
            key = f"t{table}_pre_{nprobe}_{k}"
            np.testing.assert_array_equal(I, fx[key + "_I"], err_msg=key)
            np.testing.assert_array_equal(D, fx[key + "_D"], err_msg=key)


# Distributions on which the reference's BLAS-form coarse quantizer (MKL sgemm)
# and the oracle's k-ordered fma chain give different coarse distances or
# probe lists for some query: there the end-to-end search
# is pinned as GPU = oracle (test_gpu_hard_data.py) and the reference's own
# probes feed the search_preassigned comparisons above.  tag -> number of
# (query, nprobe) probe lists that differ.
COARSE_DIFFERS = {}


def coarse_mismatch(ref, fx, xq):
    bad = 0
    for nprobe in (4, 8):
        _, _, CD, CI = ref.search(xq, 1, nprobe, nslices=1)
        same = (CI == fx[f"q{nprobe}_I"]).all(axis=1) & \
               (CD.view(np.uint32) == fx[f"q{nprobe}_D"].view(np.uint32)).all(axis=1)
        bad += int((~same).sum())
    return bad


@pytest.mark.parametrize("tag", FLAT_TAGS + PQ8_TAGS)
def test_oracle_coarse_and_search_equal_reference(amd, orc, tag):
    """quantizer->search (BLAS form) and IndexIVF::search end to end"""
    idx = amd.read_index(path(tag))
    ref = orc.IVFOracle.from_index(idx)
    fx, xq = results(tag), xq_of(tag)
    assert coarse_mismatch(ref, fx, xq) == COARSE_DIFFERS.get(tag, 0)
    if tag in COARSE_DIFFERS:
        return
    for key in [k for k in fx.files if k.startswith("full_") and k.endswith("_D")]:
        nprobe, k = map(int, key[5:-2].split("_"))
        D, I, _, _ = ref.search(xq, k, nprobe, nslices=1)
        np.testing.assert_array_equal(I, fx[key[:-2] + "_I"], err_msg=key)
        np.testing.assert_array_equal(D, fx[key], err_msg=key)


@pytest.mark.parametrize("tag", HNSW_TAGS)
def test_oracle_hnsw_equals_reference(amd, orc, tag):
    idx = amd.read_index(path(tag))
    g = orc.HNSWGraph.from_index(idx)
    fx, xq = results(tag), xq_of(tag)
    for ef in (16, 64):
        D, I = g.search(xq, 10, ef)
        np.testing.assert_array_equal(I, fx[f"ef{ef}_10_I"], err_msg=str(ef))
        np.testing.assert_array_equal(D, fx[f"ef{ef}_10_D"], err_msg=str(ef))


# ---- power-of-two scaling: exact while nothing overflows or goes subnormal
SCALE_DISTS = ["signed", "offset4", "heavy", "tight", "sparse"]


@pytest.mark.parametrize("s", [40, -40])
@pytest.mark.parametrize("dist", SCALE_DISTS)
def test_oracle_flat_is_scale_free(orc, dist, s):
    xb = hard_data.make(dist, NB, 64, SEED + 64)
    xq = IN[f"{dist}_d64_xq"]
    for metric in (1, 0):
        D, I = orc.knn(xq, xb, 10, metric=metric, blas_form=True)
        Ds, Is = orc.knn(hard_data.pow2(xq, s), hard_data.pow2(xb, s), 10, metric=metric,
                         blas_form=True)
        np.testing.assert_array_equal(Is, I)
        np.testing.assert_array_equal(Ds, D * np.float32(2.0 ** (2 * s)))


@pytest.mark.parametrize("s", [40, -40])
@pytest.mark.parametrize("tag", ["flat_l2_signed", "flat_l2_offset4", "flat_ip_heavy",
                                 "flat_l2_tight", "pq8_signed", "pq8_offset4"])
def test_oracle_ivf_is_scale_free(amd, orc, tag, s):
    """the index's centroids, rows (or PQ codebook) and the queries scaled"""
    idx = amd.read_index(path(tag))
    ref = orc.IVFOracle.from_index(idx)
    xq = xq_of(tag)
    off, codes, ids = idx.invlists_arrays()
    f = np.float32(2.0 ** s)
    if tag.startswith("pq8"):
        info = idx.pq_info()
        pq = dict(M=info["M"], nbits=info["nbits"], by_residual=info["by_residual"],
                  centroids=idx.pq_centroids * f)
        refs = orc.IVFOracle(idx.d, idx.nlist, idx.metric_type, off, codes, ids,
                             idx.quantizer.xb * f, None, pq)
    else:
        scaled = np.ascontiguousarray(codes.view(np.float32) * f).view(np.uint8)
        refs = orc.IVFOracle(idx.d, idx.nlist, idx.metric_type, off, scaled, ids,
                             idx.quantizer.xb * f)
    for k in (1, 10):
        D, I, CD, CI = ref.search(xq, k, 4, nslices=1)
        Ds, Is, CDs, CIs = refs.search(hard_data.pow2(xq, s), k, 4, nslices=1)
        np.testing.assert_array_equal(CIs, CI)
        np.testing.assert_array_equal(Is, I)
        np.testing.assert_array_equal(Ds, D * np.float32(2.0 ** (2 * s)))


@pytest.mark.parametrize("s", [40, -40])
@pytest.mark.parametrize("tag", HNSW_TAGS)
def test_oracle_hnsw_is_scale_free(amd, orc, tag, s):
    idx = amd.read_index(path(tag))
    g = orc.HNSWGraph.from_index(idx)
    ep, ml, levels, offsets, neighbors, cum = idx.graph()
    gs = orc.HNSWGraph(ep, ml, levels, offsets, neighbors, cum,
                       hard_data.pow2(idx.storage_vectors(), s))
    xq = xq_of(tag)
    D, I = g.search(xq, 10, 16)
    Ds, Is = gs.search(hard_data.pow2(xq, s), 10, 16)
    np.testing.assert_array_equal(Is, I)
    np.testing.assert_array_equal(Ds, D * np.float32(2.0 ** (2 * s)))
