"""CPU: the host restatement of IndexFlat::range_search equals the reference.

tests/golden/ref_flat_range.npz holds what the reference's
IndexFlat::range_search returned (scripts/make_golden_flat_range.py).  The
restatement (tests/flat_range_ref.py) is: the distances of
orc.knn(x, y, k = ntotal, metric, blas_form) scattered by id for the BLAS form
(>= 20 queries), orc.fvec_L2sqr / orc.fvec_inner_product per pair for the
direct form, thresholded strictly, in ascending row order.  It must give the
fixtures' lims, labels and distances bit for bit; the GPU tests
(test_gpu_flat_range.py) use it at the shapes no fixture covers."""
import numpy as np
import pytest

import flat_range_ref as fr
from flat_range_ref import CASES, load_case


@pytest.fixture(scope="module")
def gold():
    return np.load(fr.GOLD)


def test_fixture_lists_every_case(gold):
    assert sorted(str(c) for c in gold["cases"]) == sorted(CASES)


@pytest.mark.parametrize("tag", CASES)
def test_restatement_equals_reference(gold, orc, tag):
    xq, xb, ml2, radius, want = load_case(gold, orc, tag)
    got = fr.restate(orc, xq, xb, ml2, radius)
    fr.check_equal(got, want)


@pytest.mark.parametrize("tag", ["l2_d13_nq19", "ip_d40_nq19"])
def test_direct_restatement_through_knn_is_the_per_pair_one(gold, orc, tag):
    """The GPU tests' larger direct-form shapes take orc.knn(blas_form=False)
    in place of one fvec call per pair: the same distances, bit for bit."""
    xq, xb, ml2, radius, want = load_case(gold, orc, tag)
    fr.check_equal(fr.restate(orc, xq, xb, ml2, radius, per_pair=False), want)


@pytest.mark.parametrize("tag", CASES)
def test_fixture_conditions(gold, orc, tag):
    """What the generator asserted of every case still holds of the file."""
    _, nq, _, (lims, _, I) = fr.case_arrays(gold, tag)
    cnt = np.diff(lims)
    assert (cnt == 0).any()
    assert max(int(np.bincount(I[lims[i]:lims[i + 1]] // 128).max())
               for i in range(nq) if cnt[i]) > 64
    assert lims[-1] < 0.05 * nq * fr.NB
    assert (nq >= 20) == (not tag.endswith("nq19"))
