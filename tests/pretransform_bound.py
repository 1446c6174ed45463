"""How far the rounding of a linear front end can move an L2 distance; shared
by tests/test_gpu_pretransform.py and scripts/make_golden_pretransform.py.

An fp32 evaluation of xt_o = b_o + sum_j A_oj x_j, in any order, is within
e_o = (d_in + 2) 2^-24 (|b_o| + sum_j |A_oj| |x_j|) of the exact value, so two
evaluations (the reference's sgemm, this library's MFMA order) differ by at
most 2 e_o per component: a shift of the query of length at most
delta = |2 e|_2.  A squared distance dis = |xt - y|^2 then moves by at most
2 sqrt(dis) delta + delta^2."""
import numpy as np

EPS = 2.0 ** -24


def query_shift(xq, A, b):
    A64, x64 = np.abs(A.astype(np.float64)), np.abs(xq.astype(np.float64))
    e = (A.shape[1] + 2) * EPS * (np.abs(b.astype(np.float64)) + x64 @ A64.T)
    return np.linalg.norm(2 * e, axis=1)  # [nq]


def distance_move(xq, A, b, D):
    """[nq][k]: the bound for each recorded distance."""
    delta = query_shift(xq, A, b)[:, None]
    return 2 * np.sqrt(np.maximum(D.astype(np.float64), 0)) * delta + delta ** 2


def comparable(xq, A, b, D):
    """[nq] bool: every gap between consecutive recorded distances exceeds
    what the two neighbours can move together."""
    mv = distance_move(xq, A, b, D)
    gaps = np.diff(D.astype(np.float64), axis=1)
    return (gaps > mv[:, 1:] + mv[:, :-1]).all(axis=1)
