"""Named data distributions that leave the regime of float_rand (uniform in
[0, 1)): signed values, offsets that make |x|^2 + |y|^2 dwarf the distances
(cancellation, non-positive L2 approximations, margins above the k-th
distance), one dominant coordinate, near-ties under a huge margin, zero rows
and non-finite rows.  The certified bf16 filters are tested on these
(test_bf16_margin_model.py, test_gpu_hard_data.py) and the reference-run
fixtures tests/golden/ref_hard* are made from them (oracle/ref/make_golden_hard.py).

    make(name, n, d, seed)      -> float32 [n, d], the database
    queries(name, xb, nq, seed) -> float32 [nq, d], a few of them database rows
    pow2(x, s)                  -> x * 2^s (exact while nothing overflows)
"""
import numpy as np

FINITE = ["uniform", "signed", "offset1", "offset4", "offset100", "heavy", "tight", "sparse"]
NAMES = FINITE + ["nonfinite"]

HEAVY_COORD = 3        # the coordinate `heavy` multiplies by 1000
SPARSE_ZERO_ROWS = 8   # all-zero database rows of `sparse` (spread over the set)
FLT_MAX = np.finfo(np.float32).max

# `nonfinite`: (row, coordinate, value).  Row 0 is the first row of its list
# whatever the assignment; the others are ~400 rows apart, so with 8 lists they
# fall ~50 list positions apart (different 64-row tiles, checked where the
# lists are built).
NONFINITE_ROWS = [(0, 1, np.nan), (300, 7, np.nan), (700, 2, np.inf), (1100, 11, -np.inf),
                  (1500, 5, FLT_MAX), (1900, 0, -FLT_MAX)]
NONFINITE_QUERIES = [(5, 4, np.nan), (6, 9, np.inf)]


def _rng(name, seed, stream):
    return np.random.default_rng([int(seed), NAMES.index(name), stream])


def make(name, n, d, seed):
    rng = _rng(name, seed, 0)
    if name == "uniform":
        x = rng.random((n, d), np.float32)
    elif name in ("signed", "nonfinite"):
        x = rng.standard_normal((n, d), np.float32)
        if name == "nonfinite":
            for r, j, v in NONFINITE_ROWS:
                if r < n:
                    x[r, j % d] = v
    elif name.startswith("offset"):
        x = rng.random((n, d), np.float32) + np.float32(int(name[6:]))
    elif name == "heavy":
        x = rng.standard_normal((n, d), np.float32)
        x[:, HEAVY_COORD] *= np.float32(1000.0)
    elif name == "tight":
        cent = (100.0 * rng.standard_normal((64, d))).astype(np.float32)
        x = cent[np.arange(n) % 64] + (1e-3 * rng.standard_normal((n, d))).astype(np.float32)
    elif name == "sparse":
        x = rng.standard_normal((n, d), np.float32)
        x[rng.random((n, d)) < 0.9] = 0.0
        x[zero_rows(n)] = 0.0
    else:
        raise ValueError(name)
    return np.ascontiguousarray(x, dtype=np.float32)


def zero_rows(n):
    return (np.arange(SPARSE_ZERO_ROWS) * n) // SPARSE_ZERO_ROWS + 1


def clean(name, x):
    """`nonfinite` rows / queries with the altered coordinates set to 0 (what a
    k-means or a coarse assignment can be run on)."""
    x = x.copy()
    x[~np.isfinite(x) | (np.abs(x) == FLT_MAX)] = 0.0
    return x


def queries(name, xb, nq, seed):
    """Same distribution as the database (other stream); the last 4 are
    database rows (distance 0 / near-zero distances).  `sparse`: query 0 is all
    zero.  `nonfinite`: queries 5 and 6 carry a NaN and a +inf coordinate."""
    n, d = xb.shape
    rng = _rng(name, seed, 1)
    if name == "tight":
        # next to the centres the database was drawn around, not new centres
        pick = rng.integers(0, n, nq)
        xq = clean(name, xb)[pick] + (1e-3 * rng.standard_normal((nq, d))).astype(np.float32)
    else:
        xq = make(name if name != "nonfinite" else "signed", nq, d, seed + 7919)
    xq = np.ascontiguousarray(xq, dtype=np.float32)
    rows = [17, n // 3, n // 2 + 5, n - 2]   # none of them altered or zeroed
    xq[-4:] = xb[rows]
    if name == "sparse":
        xq[0] = 0.0
    if name == "nonfinite":
        for q, j, v in NONFINITE_QUERIES:
            xq[q, j % d] = v
    return xq


def pow2(x, s):
    return np.ascontiguousarray(x * np.float32(2.0 ** s), dtype=np.float32)
