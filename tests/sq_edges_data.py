"""Inputs of the IVF-SQ edge fixtures (tests/golden/ref_sq_edges*), shared by
the generator (scripts/make_golden_sq_edges.py) and the tests that rebuild the
indexes from them.

Every case is a hand-laid empty IwSq index (centroids, trained ranges, the
by-residual byte) whose lists have chosen lengths around the scan's 256-row
pass; the reference fills it with add_core.  make() derives everything from
float_rand streams (uniform [0, 1), the reference's generator) with plain fp32
arithmetic, so the arrays are the same wherever they are rebuilt; the fixture
keeps a SHA-256 of the rows the reference consumed."""
import hashlib
import struct

import numpy as np

F32 = np.float32
QT_8bit, QT_fp16 = 0, 4
LONG = [0, 1, 255, 256, 257, 513]
SHORT = [0, 1, 257]  # d = 264: keeps the files inside the size cap
NQ = 6

# tag: (qtype, metric_l2, by_residual, d, list lengths, special rows)
CASES = {
    "sq8_l2_nores_d24": (QT_8bit, 1, 0, 24, LONG, 0),
    "sq8_ip_nores_d8": (QT_8bit, 0, 0, 8, LONG, 0),
    "sq8_l2_d8": (QT_8bit, 1, 1, 8, LONG, 0),
    "sq8_ip_d264": (QT_8bit, 0, 1, 264, SHORT, 0),
    "sqfp16_ip_d8": (QT_fp16, 0, 1, 8, LONG, 0),
    "sqfp16_ip_nores_d72": (QT_fp16, 0, 0, 72, LONG, 0),
    "sqfp16_l2_nores_d264": (QT_fp16, 1, 0, 264, SHORT, 0),
    "sqfp16_l2_special_d8": (QT_fp16, 1, 1, 8, LONG, 1),
    "sqfp16_ip_special_d8": (QT_fp16, 0, 0, 8, LONG, 1),
}
TAGS = list(CASES)
PARAM_TAGS = ["sq8_l2_nores_d24", "sqfp16_ip_d8"]  # store_pairs, max_codes, selector
MAX_CODES = (1, 256, 257, 300)

# (row, component, value) of the `special` cases, rows of LONG in add order:
# list 1 is row 0, list 2 rows 1..255, list 3 256..511, list 4 512..768, list 5
# 769..1281.  Rows 1..3 are among those their list repeats at its end, so two
# rows of +inf (and of NaN) distance meet under different ids.  Stored as fp16:
# +-1e6 and 65520 (the midpoint above the largest half) become +-inf, 65519
# rounds down to 65504, 1e-7 is a subnormal half, row 800 has +inf and -inf in
# different lanes (an inner product of NaN for a query of one sign there).
SPECIAL = [
    (0, 5, -0.0), (1, 0, 1e6), (2, 1, -1e6), (3, 2, np.nan), (300, 3, 65504.0),
    (301, 3, -65504.0), (600, 4, 1e-7), (800, 0, 1e6), (800, 1, -1e6), (801, 6, 65520.0),
    (802, 6, 65519.0), (803, 5, -0.0), (1000, 7, 1e6), (1001, 7, 1e6),
]


def seed_of(tag):
    return 8300 + 10 * TAGS.index(tag)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def make(float_rand, tag):
    """float_rand(n, seed) -> n uniform floats.  Returns the case as a dict:
    cent [nlist, d], lists [nb], xb [nb, d], trained, xq [NQ, d], keys
    [NQ, nlist], cdis [NQ, nlist]."""
    qtype, l2, br, d, lens, special = CASES[tag]
    seed = seed_of(tag)
    nlist = len(lens)
    lists = np.repeat(np.arange(nlist, dtype=np.int64), lens)
    nb = lists.size
    cent = ((float_rand(nlist * d, seed).reshape(nlist, d) - F32(0.5)) * F32(2)).astype(F32)
    noise = (float_rand(nb * d, seed + 1).reshape(nb, d) - F32(0.5)).astype(F32)
    xb = (cent[lists] + F32(0.6) * noise).astype(F32)
    if special:
        for r, j, v in SPECIAL:
            xb[r, j] = v
    # the last tenth of every list repeats its first rows: ties at the k-th place
    off = np.concatenate([[0], np.cumsum(lens)])
    for l, n in enumerate(lens):
        dup = n // 10
        if dup:
            xb[off[l + 1] - dup:off[l + 1]] = xb[off[l]:off[l] + dup]
    trained = np.zeros(0, F32)
    if qtype == QT_8bit:
        # ranges from every second row only, so the other rows clamp to codes 0
        # and 255; dimension 1 is constant (vdiff == 0)
        src = (xb - cent[lists]).astype(F32) if br else xb
        vmin = src[::2].min(axis=0)
        vdiff = (src[::2].max(axis=0) - vmin).astype(F32)
        vdiff[1] = 0
        trained = np.concatenate([vmin, vdiff]).astype(F32)
    xq = ((float_rand(NQ * d, seed + 2).reshape(NQ, d) - F32(0.5)) * F32(2)).astype(F32)
    keys = np.tile(np.arange(nlist, dtype=np.int64), (NQ, 1))
    keys[1] = keys[1][::-1]     # reversed
    keys[2, 1] = -1             # an invalid probe
    keys[3, 0] = nlist - 1      # the longest list named twice
    cdis = (float_rand(NQ * nlist, seed + 3).reshape(NQ, nlist) - F32(0.5)).astype(F32)
    return dict(qtype=qtype, l2=l2, by_residual=br, d=d, lens=list(lens), nlist=nlist, nb=nb,
                cent=cent, lists=lists, xb=xb, trained=trained, xq=xq, keys=keys, cdis=cdis)


def _header(d, ntotal, trained, metric):
    return struct.pack("<iqqqBi", d, ntotal, 1 << 20, 1 << 20, trained, metric)


def empty_iwsq(d, qtype, l2, by_residual, cent, trained):
    """The bytes of an empty, trained IwSq index (faiss/impl/index_write.cpp:
    234-241, 367-389, 640-648): a flat quantizer (IxF2 / IxFI) holding cent, no
    direct map, the scalar quantizer with its trained ranges, the by-residual
    byte, and an array inverted-list block without rows."""
    nlist = cent.shape[0]
    cs = 2 * d if qtype == QT_fp16 else d
    met = 1 if l2 else 0
    b = b"IwSq" + _header(d, 0, 1, met) + struct.pack("<QQ", nlist, 1)
    b += (b"IxF2" if l2 else b"IxFI") + _header(d, nlist, 1, met)
    b += struct.pack("<Q", nlist * d) + np.ascontiguousarray(cent, F32).tobytes()
    b += struct.pack("<b", 0) + struct.pack("<Q", 0)
    b += struct.pack("<iifQQ", qtype, 0, 0.0, d, cs)
    b += struct.pack("<Q", len(trained)) + np.ascontiguousarray(trained, F32).tobytes()
    b += struct.pack("<QB", cs, int(bool(by_residual)))
    b += b"ilar" + struct.pack("<QQ", nlist, cs) + b"sprs" + struct.pack("<Q", 0)
    return b
