"""HIP path vs the reference-run fixtures on hard data (tests/golden/ref_hard*,
see tests/test_ref_hard_fixtures.py): read_index of every reference-written
file, then search_preassigned on the reference's probes and the end-to-end
search.  Ids and distances must equal the reference's arrays bit for bit on
signed, offset (cancellation), dominant-coordinate, near-tie, sparse and
non-finite data; L2 and IP IVF-Flat, d = 36, IVF-PQ 8- and 4-bit (tables 0 and
1), IVF-SQ8 and SQfp16 (signed data: a negative vmin), and HNSW.
"""
import numpy as np
import pytest

from test_ref_hard_fixtures import (ALL_TAGS, HNSW_TAGS, PQ4_TAGS, PQ8_TAGS, path,
                                    pre_cases, results, xq_of)

pytestmark = pytest.mark.gpu

IVF_TAGS = [t for t in ALL_TAGS if t not in HNSW_TAGS]


def eq(D, I, fx, key):
    np.testing.assert_array_equal(I, fx[key + "_I"], err_msg=key)
    np.testing.assert_array_equal(D.view(np.uint32), fx[key + "_D"].view(np.uint32), err_msg=key)


@pytest.mark.parametrize("tag", IVF_TAGS)
def test_gpu_preassigned_equals_reference(amd, gpu, tag):
    idx = amd.read_index(path(tag))
    fx, xq = results(tag), xq_of(tag)
    n = 0
    for key, table, nprobe, k in pre_cases(fx):
        if table is not None:
            idx.use_precomputed_table = table
        idx.nprobe = nprobe
        D, I = idx.search_preassigned(xq, k, fx[f"q{nprobe}_I"], fx[f"q{nprobe}_D"])
        eq(D, I, fx, key)
        n += 1
    assert n == (12 if tag in PQ8_TAGS + PQ4_TAGS else 6)


@pytest.mark.parametrize("tag", IVF_TAGS)
def test_gpu_coarse_and_search_equal_reference(amd, gpu, tag):
    idx = amd.read_index(path(tag))
    fx, xq = results(tag), xq_of(tag)
    for nprobe in (4, 8):
        Dq, Iq = idx.quantizer.search(xq, nprobe)
        eq(Dq, Iq, fx, f"q{nprobe}")
    for nprobe, k in ((4, 10), (8, 1)):
        idx.nprobe = nprobe
        D, I = idx.search(xq, k)
        eq(D, I, fx, f"full_{nprobe}_{k}")


@pytest.mark.parametrize("tag", HNSW_TAGS)
@pytest.mark.parametrize("q8", ["1", "0"])
def test_gpu_hnsw_equals_reference(amd, gpu, monkeypatch, tag, q8):
    monkeypatch.setenv("FAISS_AMD_HNSW_Q8", q8)
    idx = amd.read_index(path(tag))
    fx, xq = results(tag), xq_of(tag)
    for ef in (16, 64):
        idx.efSearch = ef
        D, I = idx.search(xq, 10)
        eq(D, I, fx, f"ef{ef}_10")
