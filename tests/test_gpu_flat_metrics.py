"""IndexFlat's other metrics (kernels_flat_metrics.hip) against a float64 model.

Distances: the model's value for the returned id, within (d + 4) 2^-23 sum |term|
(d terms of at most three roundings each, any order; the ratio metrics stay inside
it too); Linf exactly.  Lp / JensenShannon (device libm) get LIBM_FACTOR[metric, d]:
twice the largest error / bound measured on an MI355X where that exceeds 1.  Ids: the
float64 top-k as a set where the float64 gap between ranks k and k + 1 exceeds twice
the tolerance (at least 95 % of the queries).  DESIGN.md section 4 has the figures.
"""
import numpy as np
import pytest

from conftest import device_search

pytestmark = pytest.mark.gpu

L1, LINF, LP, CANB, BRAY, JS, JACC, NANE, ABSIP = 2, 3, 4, 20, 21, 22, 23, 24, 25
CASES = [(L1, 0), (LINF, 0), (LP, 0.5), (LP, 3), (CANB, 0), (BRAY, 0), (JS, 0), (JACC, 0),
         (NANE, 0), (ABSIP, 0)]
LIBM_FACTOR = {(JS, 1): 4670.0}  # measured 2334.9 (nearest rows of 63 on a line)
FLT_MAX = np.finfo(np.float32).max


def data(orc, m, n, d, seed):
    x = orc.float_rand(n * d, seed).reshape(n, d)
    return x + np.float32(0.25) if m in (CANB, BRAY, JS, JACC) else x - np.float32(0.5)


def model(m, arg, xq, xb):
    """float64 (value, sum |term|) of every pair, [nq][nb]"""
    x, y = xq[:, None, :].astype(np.float64), xb[None].astype(np.float64)
    a = np.abs(x - y)
    with np.errstate(invalid="ignore", divide="ignore"):
        if m == JS:
            mi = 0.5 * (x + y)
            k1, k2 = -x * np.log(mi / x), -y * np.log(mi / y)
            return 0.5 * (k1 + k2).sum(-1), 0.5 * (np.abs(k1) + np.abs(k2)).sum(-1)
        if m == NANE:  # 0 / 0 = NaN where no dimension is present in both
            v = xq.shape[1] / (~np.isnan(a)).sum(-1) * np.nansum(a * a, -1)
        else:
            v = {L1: lambda: a.sum(-1), LINF: lambda: a.max(-1), LP: lambda: (a ** arg).sum(-1),
                 CANB: lambda: (a / (np.abs(x) + np.abs(y))).sum(-1),
                 BRAY: lambda: a.sum(-1) / np.abs(x + y).sum(-1),
                 JACC: lambda: np.minimum(x, y).sum(-1) / np.maximum(x, y).sum(-1),
                 ABSIP: lambda: np.abs(x * y).sum(-1)}[m]()
    return v, np.abs(v)


def check(amd, m, arg, xb, xq, k):
    idx = amd.IndexFlat(xq.shape[1], m)
    idx.metric_arg = arg
    if len(xb):
        idx.add(xb)
    D, I = idx.search(xq, k)
    nq, nb, d = len(xq), len(xb), xq.shape[1]
    val, scale = model(m, arg, xq, xb)
    tol = (d + 4) * 2.0 ** -23 * scale * LIBM_FACTOR.get((m, d), 1.0)
    key = np.where(np.isnan(val), np.inf, -val if m == JACC else val)  # NaN never enters the heap
    order = np.argsort(key, axis=1, kind="stable")
    skipped, worst, bad = 0, 0.0, []
    for q in range(nq):
        nv = min(k, int(np.isfinite(key[q]).sum()))
        ids, o = I[q, :nv], order[q]
        assert (I[q, nv:] == -1).all() and (D[q, nv:] == (-FLT_MAX if m == JACC else FLT_MAX)).all()
        assert (ids >= 0).all() and (np.diff(key[q, ids]) >= -2 * tol[q, ids[1:]]).all()
        err, lim = np.abs(D[q, :nv] - val[q, ids]), tol[q, ids]
        worst = max(worst, (err / lim).max(initial=0))
        good = ((D[q, :nv] == val[q, ids].astype(np.float32)) if m == LINF else (err <= lim)).all()
        if nv < nb and key[q, o[nv]] - key[q, o[nv - 1]] <= 2 * max(tol[q, o[nv]], tol[q, o[nv - 1]]):
            skipped += 1
        elif set(ids) != set(o[:nv]):
            good = False
        bad += [] if good else [q]
    print(f"metric {m} arg {arg} d {d}: max error / bound {worst:.3f}, {skipped} queries skipped")
    assert not bad and skipped <= 0.05 * nq, (bad, skipped)
    return idx, D, I


# (d, ntotal, nq, k): 8-lane body, 4-step, tail; LDS slices; around the 64-wide tile
@pytest.mark.parametrize("d,nb,nq,k", [
    (1, 63, 65, 66), (7, 65, 1, 1), (8, 200, 19, 10), (12, 1, 19, 4), (33, 200, 65, 203),
    (128, 65, 65, 10), (12, 0, 3, 5)])
@pytest.mark.parametrize("m,arg", CASES)
def test_metric_against_model(gpu, amd, orc, m, arg, d, nb, nq, k):
    xb, xq = data(orc, m, nb, d, 174 + d), data(orc, m, nq, d, 274 + d)
    idx, D, I = check(amd, m, arg, xb, xq, k)
    if nq == 65:  # a pair's result does not depend on the batch around it
        D1, I1 = idx.search(xq[64:], k)
        assert np.array_equal(D1, D[64:]) and np.array_equal(I1, I[64:])
    if d == 12 and nq == 19:  # the device entry point
        Dd, Id = device_search(idx, xq, k)
        assert np.array_equal(Dd, D) and np.array_equal(Id, I)


def test_nan_euclidean_with_missing_entries(gpu, amd, orc):
    xb, xq = data(orc, NANE, 65, 12, 31), data(orc, NANE, 19, 12, 32)
    xb[::3, 2], xq[::4, 5] = np.nan, np.nan
    xq[0, :6], xb[7, 6:] = np.nan, np.nan  # no common dimension: NaN, never a result
    assert np.isnan(model(NANE, 0, xq, xb)[0][0, 7])
    _, _, I = check(amd, NANE, 0, xb, xq, 68)
    assert 7 not in I[0] and (I[0] >= 0).sum() == 64 and (I[1:] >= 0).sum() == 18 * 65


@pytest.mark.parametrize("m", [L1, LINF, ABSIP, NANE, JACC])
def test_ties_follow_the_reference_heap(gpu, amd, orc, m):  # small integers: exact in fp32
    xb, xq = [np.floor(orc.float_rand(n * 8, s) * 4).reshape(n, 8) + (m == JACC)
              for n, s in ((200, 41), (19, 42))]
    idx = amd.IndexFlat(8, m)
    idx.add(xb)
    D, I = idx.search(xq, 10)
    table = model(m, 0, xq, xb)[0].astype(np.float32)
    for q in range(19):
        Dr, Ir = orc.heap_addn_reorder(10, table[q], np.arange(200), cmax=m != JACC)
        assert np.array_equal(I[q], Ir) and np.array_equal(D[q], Dr)


@pytest.mark.parametrize("m", [L1, LINF, CANB, BRAY, JACC, NANE, ABSIP])
def test_accumulation_order_matches_the_reference(gpu, amd, orc, m):
    ref = np.load(__file__.rsplit("/", 1)[0] + "/golden/flat_metrics_ref.npz")  # the reference's D, I
    for d in (12, 33):
        idx = amd.IndexFlat(d, m)
        idx.add(data(orc, m, 200, d, 300 + d))
        D, I = idx.search(data(orc, m, 20, d, 400 + d), 10)
        assert np.array_equal(I, ref[f"I_{m}_{d}"]) and np.array_equal(D, ref[f"D_{m}_{d}"])


def test_refusals(gpu, amd, orc):
    xb = data(orc, L1, 64, 8, 51)
    idx = amd.IndexFlat(8, L1)
    idx.add(xb)
    with pytest.raises(amd.FaissError, match="selector"):
        idx.search(xb[:2], 3, params=amd.SearchParametersIVF(sel=amd.IDSelectorRange(0, 9)))
    with pytest.raises(amd.FaissError, match="metric type not supported"):
        idx.range_search(xb[:2], 1.0)
    with pytest.raises(amd.FaissError, match="coarse quantizer"):
        amd.IndexIVFFlat(idx, 8, 64).search(xb[:2], 3)
    bad = amd.IndexFlat(8, 7)
    bad.add(xb)
    with pytest.raises(amd.FaissError, match="Invalid metric 7"):
        bad.search(xb[:2], 3)
