"""The two-round certification of the IVF-Flat re-rank (ivf_rerank.h,
DESIGN.md "The exactness argument of the MFMA filters"), restated in numpy.

Every candidate carries a bracket lb' <= exact <= ub' (lb' = approx - M,
ub' = approx + M with M the margin of its probe).  Round A evaluates the
P = 16 ceil(k / 16) candidates with the smallest ub'; T = the k-th smallest
admissible exact key among them; round B evaluates the rest with lb' <= T.
Checked here, on random and on adversarial key sets:
  * the evaluated set holds every candidate whose exact key is <= the k-th
    smallest exact key of the whole stream (so the exact top-k, boundary ties
    included, is decided inside it);
  * T <= U, the k-th smallest ub' (the single sweep's threshold): round B never admits a
    candidate the single sweep would not have.
"""
import numpy as np
import pytest

FLT_MAX = float(np.finfo(np.float32).max)


def two_round(exact, lb, ub, k):
    """(evaluated set, T or None when round B's test is skipped, U)."""
    ns = len(exact)
    P = 16 * ((k + 15) // 16)
    su = np.sort(ub)
    U = su[k - 1] if ns >= k else np.inf
    A = np.argsort(ub, kind="stable")[:min(ns, P)]
    ea = exact[A]
    adm = ea[ea < FLT_MAX]  # (NaN compares false: never admissible)
    rest = np.setdiff1d(np.arange(ns), A)
    if adm.size >= k:
        T = np.sort(adm)[k - 1]
        B = rest[lb[rest] <= T]
    else:
        T = None
        B = rest
    return set(A.tolist()) | set(B.tolist()), T, U


def check(exact, lb, ub, k):
    assert np.all(lb <= exact) and np.all(exact <= ub)
    got, T, U = two_round(exact, lb, ub, k)
    adm = np.nonzero(exact < FLT_MAX)[0]
    if adm.size >= k:
        kappa = np.sort(exact[adm])[k - 1]
        need = adm[exact[adm] <= kappa]
    else:
        need = adm
    missing = set(need.tolist()) - got
    assert not missing, (k, sorted(missing))
    if T is not None:
        assert T <= U, (T, U)
    return len(got)


def brackets(rng, exact, nprobe, mscale):
    """Per-probe margins M and approximations within M of the exact keys."""
    ns = len(exact)
    probe = rng.integers(0, nprobe, ns)
    M = (mscale * (0.25 + rng.random(nprobe)))[probe]
    approx = exact + M * rng.uniform(-1.0, 1.0, ns)
    lb = np.minimum(approx - M, exact)  # (rounding of the sum, inf - inf)
    ub = np.maximum(approx + M, exact)
    inf = ~np.isfinite(exact)
    lb[inf] = exact[inf]
    ub[inf] = exact[inf]
    return lb, ub


@pytest.mark.parametrize("k", [1, 10, 16, 17, 32])
def test_random_keys(k):
    rng = np.random.default_rng(100 + k)
    rows = 0
    for trial in range(100):
        ns = int(rng.integers(k, 257))
        exact = 10.0 + 5.0 * rng.random(ns)
        lb, ub = brackets(rng, exact, 8, rng.choice([1e-3, 0.05, 0.5, 5.0]))
        rows += check(exact, lb, ub, k)
    assert rows > 0


@pytest.mark.parametrize("k", [1, 10, 16, 17, 32])
def test_duplicates_of_the_kth_value(k):
    rng = np.random.default_rng(200 + k)
    for trial in range(60):
        ns = int(rng.integers(k + 1, 257))
        exact = 10.0 + 5.0 * rng.random(ns)
        kth = np.sort(exact)[k - 1]
        dup = rng.choice(ns, size=min(ns, int(rng.integers(2, 40))), replace=False)
        exact[dup] = kth  # ties at T and across the k boundary
        lb, ub = brackets(rng, exact, 4, rng.choice([1e-3, 0.3, 3.0]))
        check(exact, lb, ub, k)


@pytest.mark.parametrize("k", [1, 10, 16, 17, 32])
def test_ns_just_above_k_and_all_equal(k):
    rng = np.random.default_rng(300 + k)
    for ns in (k, k + 1, k + 2, 16 * ((k + 15) // 16) + 1):
        for trial in range(20):
            exact = 1.0 + rng.random(ns)
            lb, ub = brackets(rng, exact, 3, 0.4)
            check(exact, lb, ub, k)
            same = np.full(ns, 7.25)
            lb, ub = brackets(rng, same, 3, rng.choice([0.0, 0.4]))
            # every candidate ties with the k-th: all of them are needed
            assert check(same, lb, ub, k) == ns


@pytest.mark.parametrize("k", [1, 10, 16, 17, 32])
def test_inf_entries(k):
    rng = np.random.default_rng(400 + k)
    for trial in range(60):
        ns = int(rng.integers(k, 200))
        exact = 3.0 + rng.random(ns)
        ninf = int(rng.integers(1, ns + 1))  # up to all of them: fewer than k admissible
        exact[rng.choice(ns, size=ninf, replace=False)] = np.inf
        lb, ub = brackets(rng, exact, 5, rng.choice([0.01, 0.5]))
        check(exact, lb, ub, k)


def test_second_round_is_tighter_than_one_sweep():
    """The point of the change: with margins of the size of the spread of the
    keys, the two rounds evaluate clearly fewer rows than `lb' <= U` does."""
    rng = np.random.default_rng(5)
    k, one, two = 10, 0, 0
    for trial in range(60):
        exact = 10.0 + 5.0 * rng.random(256)
        lb, ub = brackets(rng, exact, 8, 0.2)
        U = np.sort(ub)[k - 1]
        one += int((lb <= U).sum())
        two += check(exact, lb, ub, k)
    assert two < one
