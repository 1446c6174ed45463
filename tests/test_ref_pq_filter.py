"""CPU checks against the reference-run fixtures tests/golden/ref_pq_filter*
(scripts/make_golden_pq_filter.py): the four 8-bit IVF-PQ geometries of the
MFMA filter that ref_full does not hold (M32 d64, M12 d96, M64 d128, M16 d128),
over base rows with repeated vectors and permuted ids.

As tests/test_ref_fixtures.py does for ref_full: the product's reader parses
the reference-written files (same lists, same bytes written back), and the
oracle restatement over them reproduces every recorded D and I bit for bit —
search_preassigned for both precomputed-table settings at k = 1, 10, 20, and
the search with max_codes and an IDSelectorBatch.  This is what lets
tests/test_gpu_pq_filter_edges.py hold the GPU to the oracle at these
geometries.
"""
import hashlib
import os

import numpy as np
import pytest

import pq_filter_data as pf

HERE = os.path.dirname(os.path.abspath(__file__))
GDIR = os.path.join(HERE, "golden", "ref_pq_filter")
FX = np.load(os.path.join(HERE, "golden", "ref_pq_filter.npz"))
TAGS = list(pf.REF_TAGS)


def path(tag):
    return os.path.join(GDIR, tag + ".faiss")


@pytest.mark.parametrize("tag", TAGS)
def test_read_reference_file(amd, tag):
    idx = amd.read_index(path(tag))
    info = FX[tag + "_info"]
    d, M = pf.REF_TAGS[tag]
    assert (idx.d, idx.ntotal, idx.nlist) == (d, pf.REF_NB, pf.REF_NLIST) == tuple(info[[0, 1, 3]])
    assert idx.metric_type == 1 == info[2] and idx.code_size == M == info[5]
    pi = idx.pq_info()
    assert pi["M"] == M == info[6] and pi["nbits"] == 8 == info[7]
    assert pi["by_residual"] == 1 == info[8]
    sizes = np.array([idx.get_list_size(l) for l in range(idx.nlist)], np.int64)
    sha = hashlib.sha256()
    for l in range(idx.nlist):
        sha.update(np.ascontiguousarray(idx.list_codes(l), np.uint8).tobytes())
        sha.update(np.ascontiguousarray(idx.list_ids(l), np.int64).tobytes())
    np.testing.assert_array_equal(sizes, FX[tag + "_sizes"])
    np.testing.assert_array_equal(np.frombuffer(sha.digest(), np.uint8), FX[tag + "_sha"])


@pytest.mark.parametrize("tag", TAGS)
def test_rewrite_reference_file_byte_identical(amd, tag, tmp_path):
    out = str(tmp_path / "re.faiss")
    amd.write_index(amd.read_index(path(tag)), out)
    with open(path(tag), "rb") as f1, open(out, "rb") as f2:
        assert f1.read() == f2.read()


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_inputs_are_the_planted_ones(amd, orc, tag):
    """The recorded queries and selector are pq_filter_data.ref_inputs' (the
    generator's inputs), codes repeat inside the lists, and the ids are not
    in arrival order."""
    c = pf.ref_inputs(orc.float_rand, tag)
    np.testing.assert_array_equal(c["xq"], FX[tag + "_xq"])
    np.testing.assert_array_equal(c["sel"], FX[tag + "_params_sel"])
    assert 0.35 < c["sel"].size / pf.REF_NB < 0.45
    idx = amd.read_index(path(tag))
    off, codes, ids = idx.invlists_arrays()
    assert sorted(ids.tolist()) == sorted(c["ids"].tolist())
    assert (np.diff(ids[off[0]:off[1]]) < 0).any()
    groups = np.unique(codes, axis=0, return_counts=True)[1]
    assert (groups >= pf.REF_COPIES).sum() >= pf.REF_NREP


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_preassigned_equals_reference(amd, orc, tag):
    idx = amd.read_index(path(tag))
    ref = orc.IVFOracle.from_index(idx)
    xq = FX[tag + "_xq"]
    tied = 0
    for table in (1, 0):
        ref.use_precomputed_table = table
        for nprobe, k in pf.REF_CASES:
            key = f"{tag}_t{table}_pre_{nprobe}_{k}"
            D, I = ref.search_preassigned(xq, k, FX[f"{tag}_q{nprobe}_I"], FX[f"{tag}_q{nprobe}_D"])
            np.testing.assert_array_equal(I, FX[key + "_I"], err_msg=key)
            np.testing.assert_array_equal(D, FX[key + "_D"], err_msg=key)
            if k > 1:
                tied += int((D[:, 0] == D[:, k - 1]).sum())
    # the copies of a repeated vector share a code: their group is cut at k
    assert tied >= 6 * pf.REF_NREP


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_coarse_equals_reference(amd, orc, tag):
    idx = amd.read_index(path(tag))
    ref = orc.IVFOracle.from_index(idx)
    for nprobe in (5, 8, 16):
        _, _, CD, CI = ref.search(FX[tag + "_xq"], 1, nprobe, nslices=1)
        np.testing.assert_array_equal(CI, FX[f"{tag}_q{nprobe}_I"])
        np.testing.assert_array_equal(CD, FX[f"{tag}_q{nprobe}_D"])


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_max_codes_selector_equals_reference(amd, orc, tag):
    idx = amd.read_index(path(tag))
    pr = pf.REF_PARAMS
    keys, cdis = FX[f"{tag}_q{pr['nprobe']}_I"], FX[f"{tag}_q{pr['nprobe']}_D"]
    D, I = pf.oracle_params_search(orc, idx, FX[tag + "_xq"], pr["k"], keys, cdis,
                                   pr["max_codes"], FX[tag + "_params_sel"], table=1)
    np.testing.assert_array_equal(I, FX[tag + "_params_I"])
    np.testing.assert_array_equal(D, FX[tag + "_params_D"])
    # the cap bites: without it the result differs
    D0, I0 = pf.oracle_params_search(orc, idx, FX[tag + "_xq"], pr["k"], keys, cdis, 0,
                                     FX[tag + "_params_sel"], table=1)
    assert (I0 != I).any()
