"""The certificate of the bf16 MFMA filters restated in numpy, in the style of
test_hnsw_q8_bound.py: for every pair (query, row) of every finite
distribution of tests/hard_data.py

    |approx - exact| <= margin      and, through the 32-bit key truncation,
    decode_lo - margin <= exact <= decode_hi + margin.

approx is the filter's value: operands split into bf16 parts by
round-to-nearest-even on the bit pattern, the parts' products exact, summed in
fp32 along k (forward, reverse and pairwise: the certificate must not depend
on the MFMA's internal order).  exact is the reference's fp32 evaluation
(ref_arith.h order; for the coarse quantizer also the BLAS form).  The margins
and coefficients are restated once below, each beside the source line it
restates.  The file also asserts the regimes the distributions are meant to
reach, so that the GPU tests over them cannot test nothing.
"""
import numpy as np
import pytest

import hard_data

F32 = np.float32
U24 = 1.0 / 16777216.0
DIMS = [36, 64, 128]
DISTS = hard_data.FINITE


# ------------------------------------------------------------------ the code's formulas
def ivf_bf3_coef(d):    # kernels_ivf_mfma.hip:917-920
    return 2.0 * (3.1 / 65536.0 + (6.0 * d + 8.0) * U24)


def ivf_bf3f_coef(d):   # kernels_ivf_mfma.hip:929-932
    return 2.0 * (3.1 / 65536.0 + (9.1 * d + 24.0) * U24)


def ivf_bf2_coef(d):    # kernels_ivf_mfma.hip:934-937
    return 1.02 / 65536.0 + (6.1 * d + 8.0) * U24


def ivf_bf2f_coef(d):   # kernels_ivf_mfma.hip:943-946
    return 1.02 / 65536.0 + (9.1 * d + 24.0) * U24


def ivfpq_mfma_coef(d, M):  # kernels_pq_mfma.hip:83-88
    return 1.02 / 65536.0 + (4.0 * d + 2.0 * M + 64.0) * U24


def ivf_bf3_obits(max_list_len):  # kernels_ivf_mfma.hip:910-915
    tiles = max(1, (max_list_len + 63) // 64)
    b = 0
    while (1 << b) < tiles:
        b += 1
    return 4 + b


def margin_y3(coef, xn, yn):
    # kernels_ivf_mfma.hip:295 (Y3) and kernels_coarse.hip:80
    return (F32(coef) * (xn + yn) + F32(1e-30)).astype(F32)


def margin_bf2(coef, xn, yn, rres):
    # kernels_ivf_mfma.hip:296-297, :683 and kernels_coarse.hip:81
    return (F32(2) * (F32(2) * np.sqrt(xn) * rres + F32(coef) * (xn + yn)) + F32(1e-30)).astype(F32)


def margin_pq(coef, xn, cnorm, R, r):
    # kernels_ivf_mfma.hip:679-681 and kernels_pq_mfma.hip:375, :612
    xl = np.sqrt(xn)
    sr = (xl + cnorm + R).astype(F32)
    return (F32(2) * (F32(2) * xl * r + F32(coef) * sr * sr) + F32(1e-30)).astype(F32)


def row_resnorm(y):
    # kernels_ivf_mfma.hip:949-960 (k_row_resnorm)
    e = y.astype(np.float64) - bf16(y).astype(np.float64)
    return (F32(1) * (np.sqrt((e * e).sum(-1)) * (1.0 + 1e-6)).astype(F32) + F32(1e-38)).astype(F32)


# ------------------------------------------------------------------ number formats
def bf16(x):
    """float32 -> nearest bf16 (ties to even on the bit pattern), as float32"""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7fff)
    return ((u + r) & np.uint32(0xffff0000)).view(F32)


def split2(x):
    h = bf16(x)
    return h, bf16((x - h).astype(F32))


def split3(x):  # bf3.h:125-130
    h = bf16(x)
    r1 = (x - h).astype(F32)
    m = bf16(r1)
    return h, m, bf16((r1 - m).astype(F32))


def fma(a, b, c):
    """one rounding (the product of two float32 is exact in float64)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def accumulate(terms, order):
    """fp32 sum of exact products along the last axis"""
    t = terms.astype(F32)
    if order == "reverse":
        t = t[..., ::-1]
    if order == "pairwise":
        n = 1 << (t.shape[-1] - 1).bit_length()
        t = np.concatenate([t, np.zeros(t.shape[:-1] + (n - t.shape[-1],), F32)], -1)
        while t.shape[-1] > 1:
            t = (t[..., 0::2] + t[..., 1::2]).astype(F32)
        return t[..., 0]
    acc = np.zeros(t.shape[:-1], F32)
    for j in range(t.shape[-1]):
        acc = (acc + t[..., j]).astype(F32)
    return acc


def norm_seq(x):
    acc = np.zeros(x.shape[:-1], F32)
    for j in range(x.shape[-1]):
        acc = fma(x[..., j], x[..., j], acc)
    return acc


# ------------------------------------------------------------------ the exact side
def ref_dist(x, y, l2):
    """ref_arith.h ref_dist<L2> for all pairs: x [nq, d], y [nb, d] -> [nq, nb]"""
    d = x.shape[1]
    X, Y = x[:, None, :], y[None, :, :]

    def term_fma(i, acc):
        if l2:
            t = (X[..., i] - Y[..., i]).astype(F32)
            return fma(t, t, acc)
        return fma(X[..., i] + F32(0) * Y[..., i], Y[..., i] + F32(0) * X[..., i], acc)

    def term(i):
        if l2:
            t = (X[..., i] - Y[..., i]).astype(F32)
            return (t * t).astype(F32)
        return (X[..., i] * Y[..., i]).astype(F32)

    n8 = d & ~7
    c = [np.zeros((x.shape[0], y.shape[0]), F32) for _ in range(8)]
    for i in range(0, n8, 8):
        for j in range(8):
            c[j] = term_fma(i + j, c[j])
    x0, x1, x2, x3 = ((c[j] + c[j + 4]).astype(F32) for j in range(4))
    r = ((x0 + x2).astype(F32) + (x1 + x3).astype(F32)).astype(F32)
    i = n8
    if d - n8 >= 4:
        e = [term(i + j) for j in range(4)]
        r = (r + ((e[0] + e[2]).astype(F32) + (e[1] + e[3]).astype(F32)).astype(F32)).astype(F32)
        i += 4
    for j in range(i, d):
        r = term_fma(j, r)
    return r


def blas_l2(x, y):
    """the coarse quantizer's form: fma(-2, <x, y> (k-ordered fma chain),
    |x|^2 + |y|^2), clamped at 0"""
    ip = np.zeros((x.shape[0], y.shape[0]), F32)
    for j in range(x.shape[1]):
        ip = fma(x[:, None, j] + F32(0) * ip, y[None, :, j] + F32(0) * ip, ip)
    s = (norm_seq(x)[:, None] + norm_seq(y)[None, :]).astype(F32)
    return np.maximum(fma(np.full_like(ip, -2), ip, s), F32(0))


# ------------------------------------------------------------------ the approx side
def products(x, y, form):
    """the exact products a filter accumulates, in the kernel's k order:
    [nq, nb, terms]"""
    xh, xl = split2(x)
    yh, yl = split2(y)
    X = lambda a: a[:, None, :]  # noqa: E731
    Y = lambda a: a[None, :, :]  # noqa: E731
    if form.startswith("bf16x3"):   # bf3.h:223-227 (bf3_block)
        parts = [Y(yl) * X(xh), Y(yh) * X(xl), Y(yh) * X(xh)]
    else:                           # bf3.h:242-245 (bf2_block)
        parts = [Y(yh) * X(xl), Y(yh) * X(xh)]
    t = np.stack(parts, -1).reshape(x.shape[0], y.shape[0], -1)
    if form.endswith("fold"):
        # the bias k-step (kernels_ivf_mfma.hip:350-355, :474-488):
        # A = {-|y|^2/2 in three bf16 parts, 1, 1, 1}, B = {1, 1, 1, -|x|^2/2 in three}
        yb = np.stack(split3((F32(-0.5) * norm_seq(y)).astype(F32)), -1)
        xb = np.stack(split3((F32(-0.5) * norm_seq(x)).astype(F32)), -1)
        bias = np.concatenate([np.broadcast_to(yb[None], (x.shape[0],) + yb.shape),
                               np.broadcast_to(xb[:, None], (x.shape[0], y.shape[0], 3))], -1)
        t = np.concatenate([t, bias], -1)
    return t


def approx_and_key(x, y, form, l2, order):
    """(raw approx, key bits, fold flag) of every pair"""
    acc = accumulate(products(x, y, form), order)
    if form.endswith("fold"):
        return (F32(-2) * acc).astype(F32), acc.view(np.uint32), True   # bf3.h:95
    if l2:   # kernels_ivf_mfma.hip:243 / :624
        s = (norm_seq(x)[:, None] + norm_seq(y)[None, :]).astype(F32)
        a = fma(np.full_like(acc, -2), acc, s)
        return a, np.maximum(a, F32(0)).view(np.uint32), False          # bf3.h:60
    a = (F32(0) - acc).astype(F32)
    u = a.view(np.uint32)                                               # wave_select.h:157-160
    key = u ^ ((u.view(np.int32) >> 31).view(np.uint32) | np.uint32(0x80000000))
    return a, key, False


def decode(key, mask, l2, fold):
    """(lo, hi) of bf3.h:75-81 (plain) / :108-113 (folded)"""
    lo, hi = key & ~np.uint32(mask), key | np.uint32(mask)
    if fold:
        return (np.maximum(F32(-2) * lo.view(F32), F32(0)),
                np.maximum(F32(-2) * hi.view(F32), F32(0)))
    if l2:
        return lo.view(F32), hi.view(F32)

    def un(u):                                                          # wave_select.h:161-163
        return (u ^ (~(u.view(np.int32) >> 31).view(np.uint32) | np.uint32(0x80000000))).view(F32)
    return un(lo), un(hi)


def margins(x, y, form, d):
    xn, yn = norm_seq(x)[:, None], norm_seq(y)[None, :]
    if form == "bf16x3":
        return margin_y3(ivf_bf3_coef(d), xn, yn)
    if form == "bf16x3fold":
        return margin_y3(ivf_bf3f_coef(d), xn, yn)
    coef = ivf_bf2f_coef(d) if form == "bf16x2fold" else ivf_bf2_coef(d)
    return margin_bf2(coef, xn, yn, row_resnorm(y)[None, :])


FORMS = [("bf16x2", True), ("bf16x2", False), ("bf16x3", True), ("bf16x3", False),
         ("bf16x2fold", True), ("bf16x3fold", True)]
_data = {}


def data(dist, d, nb=384, nq=12):
    if (dist, d, nb) not in _data:
        xb = hard_data.make(dist, nb, d, 31 + d)
        _data[(dist, d, nb)] = (xb, hard_data.queries(dist, xb, nq, 31 + d))
    return _data[(dist, d, nb)]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dist", DISTS)
def test_flat_and_coarse_certificate(dist, d):
    xb, xq = data(dist, d)
    exact = {True: [ref_dist(xq, xb, True), blas_l2(xq, xb)],
             False: [(F32(0) - ref_dist(xq, xb, False)).astype(F32)]}
    worst = {}
    for form, l2 in FORMS:
        m = margins(xq, xb, form, d).astype(np.float64)
        for order in ("forward", "reverse", "pairwise"):
            a, key, fold = approx_and_key(xq, xb, form, l2, order)
            for ex in exact[l2]:
                ex = ex.astype(np.float64)
                # the clamp is part of the argument: exact L2 distances are >= 0
                mid = np.maximum(a, F32(0)).astype(np.float64) if l2 else a.astype(np.float64)
                ratio = np.abs(mid - ex) / m
                worst[(form, l2)] = max(worst.get((form, l2), 0.0), float(ratio.max()))
                assert (ratio <= 1.0).all(), (dist, d, form, l2, order, float(ratio.max()))
                for obits in (4, 6, 10):
                    lo, hi = decode(key, (1 << obits) - 1, l2, fold)
                    assert (lo.astype(np.float64) - m <= ex).all(), (dist, d, form, l2, obits)
                    assert (ex <= hi.astype(np.float64) + m).all(), (dist, d, form, l2, obits)
    print(f"{dist} d={d} max |approx - exact| / margin: " +
          ", ".join(f"{f}/{'L2' if l else 'IP'} {v:.3f}" for (f, l), v in worst.items()))


@pytest.mark.parametrize("dist", DISTS)
def test_pq_certificate(dist):
    """k_ivfpq_filter_w's form: rows y_C + y_R with y_R decoded from a random
    codebook (M = 16, dsub = 4), approx = coarse_dis + term - 2 <xh + xl,
    bf16(y_R)>, term = |y_R|^2 + 2 <y_C, y_R>; exact = the reference's table-0
    sum of per-subquantizer fp32 distances of the residual x - y_C."""
    d, M, ds = 64, 16, 4
    xb, xq = data(dist, d)
    rng = np.random.default_rng(5)
    cent = xb[rng.choice(xb.shape[0], 8, replace=False)]
    res = (xb - cent[rng.integers(0, 8, xb.shape[0])]).astype(F32)
    book = np.stack([res[rng.choice(res.shape[0], 256), m * ds:(m + 1) * ds] for m in range(M)])
    coef = ivfpq_mfma_coef(d, M)
    for l in range(0, 8, 3):
        codes = rng.integers(0, 256, (128, M))
        yr = np.concatenate([book[m, codes[:, m]] for m in range(M)], 1).astype(F32)
        yc = cent[l]
        cd = ref_dist(xq, yc[None], True)                       # coarse_dis [nq, 1]
        term = fma(np.full(128, 2, F32), ref_dist(yc[None], yr, False)[0], norm_seq(yr))
        xh, xl = split2(xq)
        yh = bf16(yr)
        t = np.stack([yh[None] * xl[:, None], yh[None] * xh[:, None]], -1).reshape(
            xq.shape[0], 128, -1)
        r = (xq - yc).astype(F32)
        ex = np.zeros((xq.shape[0], 128), F32)
        for m in range(M):                                      # the sequential LUT sum
            sl = slice(m * ds, (m + 1) * ds)
            sub = np.zeros_like(ex)
            for j in range(m * ds, (m + 1) * ds):
                tt = (r[:, None, j] - yr[None, :, j]).astype(F32)
                sub = (sub + (tt * tt).astype(F32)).astype(F32)
            ex = (ex + sub).astype(F32)
        R = (np.sqrt((yr.astype(np.float64) ** 2).sum(1)) * (1 + 1e-6)).astype(F32)  # pq_mfma:67
        e = yr.astype(np.float64) - yh.astype(np.float64)
        rr = (np.sqrt((e * e).sum(1)) * (1 + 1e-6)).astype(F32)                      # pq_mfma:68
        cn = F32(np.sqrt((yc.astype(np.float64) ** 2).sum()))
        m_ = margin_pq(coef, norm_seq(xq)[:, None], cn, R[None], rr[None]).astype(np.float64)
        for order in ("forward", "reverse", "pairwise"):
            acc = accumulate(t, order)
            a = np.maximum(fma(np.full_like(acc, -2), acc, (cd + term[None]).astype(F32)), F32(0))
            ratio = np.abs(a.astype(np.float64) - ex.astype(np.float64)) / m_
            assert (ratio <= 1.0).all(), (dist, l, order, float(ratio.max()))


# ------------------------------------------------------------------ regimes
def window(dist, nb=4096, nq=16, d=64, k=10):
    """the bf16x2 filter over all rows as one probed list: the share of
    candidates the certificate cannot drop (lb' <= U, U = k-th smallest ub'),
    the share of non-positive approximations, and margin / k-th distance"""
    xb, xq = data(dist, d, nb, nq)
    a, _, _ = approx_and_key(xq, xb, "bf16x2", True, "forward")
    xn = norm_seq(xq)[:, None]
    mm = margin_bf2(ivf_bf2_coef(d), xn, norm_seq(xb).max(), row_resnorm(xb).max())
    key = np.maximum(a, F32(0))
    U = np.sort(key + mm, axis=1)[:, k - 1:k]
    kth = np.sort(ref_dist(xq, xb, True), axis=1)[:, k - 1]
    return float((key - mm <= U).mean()), float((a <= 0).mean()), float((mm[:, 0] / kth).min())


def test_regime_uniform_is_the_easy_case():
    share, nonpos, _ = window("uniform")
    assert share < 0.02 and nonpos < 0.001, (share, nonpos)


def test_regime_offset1_partial_window():
    share, _, _ = window("offset1")
    assert 0.02 <= share <= 0.50, share


@pytest.mark.parametrize("dist", ["offset4", "offset100"])
def test_regime_offsets_margin_above_kth_distance(dist):
    share, nonpos, m_over_kth = window(dist)
    assert share == 1.0 and m_over_kth > 1.0, (share, m_over_kth)
    if dist == "offset100":
        assert nonpos > 0.25, nonpos


def test_regime_signed_ip_keys_of_both_signs():
    xb, xq = data("signed", 64, 4096, 16)
    ip = ref_dist(xq, xb, False)
    assert ((ip > 0).any(axis=1) & (ip < 0).any(axis=1)).all()


def test_regime_heavy_cauchy_schwarz_term_dominates():
    xb, xq = data("heavy", 64)
    xn, yn = norm_seq(xq)[:, None], norm_seq(xb)[None, :]
    cs = F32(4) * np.sqrt(xn) * row_resnorm(xb)[None, :]
    assert (cs > 0.5 * margin_bf2(ivf_bf2_coef(64), xn, yn, row_resnorm(xb)[None, :])).mean() > 0.9


def test_regime_tight_near_ties_not_ties():
    xb, xq = data("tight", 64, 4096, 16)
    dis = np.sort(ref_dist(xq, xb, True), axis=1)[:, :10]
    gaps = np.diff(dis, axis=1)
    mm = margin_bf2(ivf_bf2_coef(64), norm_seq(xq), norm_seq(xb).max(), row_resnorm(xb).max())
    assert (gaps > 0).mean() > 0.9 and dis[:, 9].max() < 1e-2 and mm.min() > 1.0


def test_regime_sparse_zero_rows_and_query():
    xb, xq = data("sparse", 64, 4096, 16)
    # (0.9^64: a few more rows come out all zero by chance)
    assert (norm_seq(xb) == 0).sum() >= hard_data.SPARSE_ZERO_ROWS and norm_seq(xq)[0] == 0
    assert (norm_seq(xb[hard_data.zero_rows(4096)]) == 0).all()
    assert ((ref_dist(xq, xb, False) == 0).sum(axis=1) >= hard_data.SPARSE_ZERO_ROWS).all()


@pytest.mark.parametrize("s", [40, -40])
@pytest.mark.parametrize("dist", DISTS)
def test_pow2_scaling_stays_finite_and_normal(dist, s):
    xb, _ = data(dist, 64)
    n = norm_seq(hard_data.pow2(xb, s))
    tiny = np.finfo(np.float32).tiny
    assert np.isfinite(n).all() and ((n == 0) | (n >= tiny)).all()


def test_obits_of_the_test_lists():
    assert [ivf_bf3_obits(n) for n in (1, 64, 65, 256, 300, 2048)] == [4, 4, 5, 6, 7, 9]
