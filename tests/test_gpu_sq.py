"""IndexIVFScalarQuantizer search on the GPU against reference runs.

Every expected array in tests/golden/ref_sq.npz was produced by the reference
library (scripts/make_golden_sq.py) over the index files in
tests/golden/ref_sq/.  Ids and distances must be equal bit for bit: the scan
kernel (csrc/kernels_sq.hip) restates the reference's fp32 evaluation order
(csrc/sq_ref.h) and the exact select reproduces its heap."""
import os

import numpy as np
import pytest

from conftest import assert_same_results, device_search

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = ["sq8_l2_d64", "sq8_l2_d72", "sqfp16_l2_d64", "sq8_ip_d64", "sq8_hnsw_d64"]
PAIR_TAGS = ["sq8_l2_d64", "sq8_ip_d64"]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_sq.npz"))


@pytest.fixture(scope="module")
def indexes(amd, gpu):
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = amd.read_index(os.path.join(HERE, "golden", "ref_sq", tag + ".faiss"))
        return cache[tag]
    return get


@pytest.mark.parametrize("tag", TAGS)
def test_search_preassigned(indexes, fx, tag):
    idx = indexes(tag)
    xq = fx[f"{tag}_xq"]
    nlist = int(fx[f"{tag}_meta"][1])
    for nprobe in (1, 4, nlist):
        Iq, Dq = fx[f"{tag}_q{nprobe}_I"].astype(np.int64), fx[f"{tag}_q{nprobe}_D"]
        idx.nprobe = nprobe
        for k in (1, 10, 100):
            D, I = idx.search_preassigned(xq, k, Iq, Dq)
            assert_same_results(D, I, fx[f"{tag}_pre_{nprobe}_{k}_D"],
                                fx[f"{tag}_pre_{nprobe}_{k}_I"].astype(np.int64))


@pytest.mark.parametrize("tag", TAGS)
def test_search_end_to_end(indexes, fx, tag):
    idx = indexes(tag)
    xq = fx[f"{tag}_xq"]
    idx.nprobe = 4
    Dr, Ir = fx[f"{tag}_full_4_10_D"], fx[f"{tag}_full_4_10_I"].astype(np.int64)
    D, I = idx.search(xq, 10)
    assert_same_results(D, I, Dr, Ir)
    Dd, Id = device_search(idx, xq, 10)
    assert_same_results(Dd, Id, D, I)


@pytest.mark.parametrize("tag", PAIR_TAGS)
def test_store_pairs(indexes, fx, tag):
    idx = indexes(tag)
    idx.nprobe = 4
    D, I = idx.search_preassigned(fx[f"{tag}_xq"], 10, fx[f"{tag}_q4_I"].astype(np.int64),
                                  fx[f"{tag}_q4_D"], store_pairs=True)
    assert_same_results(D, I, fx[f"{tag}_sp_D"], fx[f"{tag}_sp_I"])
    lists = I[I >= 0] >> 32
    assert lists.min() >= 0 and lists.max() < idx.nlist


@pytest.mark.parametrize("tag", PAIR_TAGS)
def test_max_codes_and_selector(amd, indexes, fx, tag):
    idx = indexes(tag)
    nb = int(fx[f"{tag}_meta"][2])
    sel = amd.IDSelectorBatch((np.arange(nb, dtype=np.int64) * 3 + 7)[::2])
    params = amd.SearchParametersIVF(nprobe=8, max_codes=300, sel=sel)
    D, I = idx.search(fx[f"{tag}_xq"], 10, params=params)
    assert_same_results(D, I, fx[f"{tag}_params_D"], fx[f"{tag}_params_I"].astype(np.int64))


def test_all_rows_d72(indexes, fx):
    """nprobe = nlist, k = nb: the result holds every row's distance, so each
    row's arithmetic is compared with the reference's (rows of 72 bytes: the
    last 16-byte load of a row is half used)."""
    tag = "sq8_l2_d72"
    idx = indexes(tag)
    nlist, nb = int(fx[f"{tag}_meta"][1]), int(fx[f"{tag}_meta"][2])
    xq = fx[f"{tag}_xq"][:20]
    idx.nprobe = nlist
    D, I = idx.search_preassigned(xq, nb, fx[f"{tag}_q{nlist}_I"][:20].astype(np.int64),
                                  fx[f"{tag}_q{nlist}_D"][:20])
    Dr, Ir = fx[f"{tag}_all_D"], fx[f"{tag}_all_I"].astype(np.int64)
    assert (Ir >= 0).all()
    assert_same_results(D, I, Dr, Ir)
