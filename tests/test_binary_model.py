"""tests/binary_model.py against the reference's recorded results
(scripts/make_golden_binary.py): d = 16, 300 rows, so nearly every k boundary
falls inside a tie group; the IVF ids are shuffled, so they do not ascend along
the arrival order.  This pins the three result rules."""
import os

import numpy as np
import pytest

import binary_model as bm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_binary")
TAGS = ["flat_heap", "flat_count", "ivf_heap", "ivf_count", "ivf_heap_mc64", "ivf_count_mc64"]


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_binary.npz"))


@pytest.mark.parametrize("tag", TAGS)
def test_model_reproduces_reference(ref, tag):
    heap, nprobe, mc = (int(v) for v in ref[tag + "_cfg"])
    k = int(ref["k"])
    if tag.startswith("flat"):
        D, I = bm.flat_search(ref["xb"], ref["xq"], k)
    else:
        model = bm.IVFModel(ref["cent"], ref["xb"], ref["ids"])
        D, I = model.search(ref["xq"], k, nprobe, use_heap=bool(heap), max_codes=mc)
    assert np.array_equal(D, ref[tag + "_D"]) and np.array_equal(I, ref[tag + "_I"])


def test_fixture_has_descending_ids_and_boundary_ties(ref):
    model = bm.IVFModel(ref["cent"], ref["xb"], ref["ids"])
    assert any((np.diff(ref["ids"][model.arrivals(q, 3)]) < 0).any() for q in ref["xq"])
    # the two IVF rules differ on these data, so the fixtures tell them apart
    assert not np.array_equal(ref["ivf_heap_I"], ref["ivf_count_I"])
    # the k-th distance is shared past the boundary for most queries
    k = int(ref["k"])
    dis = bm.hamming(ref["xq"], ref["xb"])
    tied = [(np.sort(row)[k - 1] == np.sort(row)[k]) for row in dis]
    assert sum(tied) >= len(tied) // 2
