"""numpy restatement of the reference's IVF-PQ search for packed codes
(4 <= nbits < 8), the rule csrc/pq_ref.h and csrc/kernels_exact.hip state in HIP.

* Codes: the little-endian bit stream of PQEncoderGeneric / PQDecoderGeneric
  (faiss/impl/ProductQuantizer-inl.h:10-97), index m in bits [m nbits, (m+1) nbits).
* Table entries: fvec_inner_products_ny / fvec_L2sqr_ny for dsub 1 / 2 / 4 / 8
  (faiss/utils/distances_simd.cpp): the first term rounded, then an fma chain.
* Tables (faiss/IndexIVFPQ.cpp:545-700): table 0 (by residual, L2) is
  |r_m - c|^2 of the residual r = x - y_C with dis0 = 0; table 1 is
  fma(-2, <x_m, c>, P), P = fma(2, <y_C,m, c>, |c|^2), with dis0 = the coarse
  distance; inner product is <x_m, c> with dis0 = <x, y_C>; not by residual
  is the table of x itself with dis0 = 0.
* Code sum: every decoder but PQDecoder8 takes distance_single_code_generic
  (faiss/impl/code_distance/code_distance-generic.h:16-79), the plain chain
  r = 0; r += tab[m][idx_m]; the distance is dis0 + r.
* Heap: a row is admitted when its distance strictly beats the heap's top
  (faiss/IndexIVFPQ.cpp:760-778); the heap orders (distance, id) pairs
  (faiss/utils/Heap.h cmp2), so it evicts the worst pair and heap_reorder
  returns the pairs best first.  Rows arrive probe by probe in list order.
* Range (faiss/IndexIVFPQ.cpp:780-799): kept when dis < radius (L2) or
  dis > radius (inner product), in arrival order.

fp32 throughout; fma() is correctly rounded (round-to-odd in float64)."""
import bisect

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def fma(a, b, c):
    """Correctly rounded fp32 a * b + c.  The product of two fp32 values is
    exact in float64; the float64 sum is rounded to odd (its error is recovered
    with a two-sum) so that the final rounding to fp32 is the only one."""
    a = np.asarray(a, F32).astype(np.float64)
    b = np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    s, err = np.broadcast_arrays(s, err)
    s = s.copy()
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s[fix] = np.nextafter(s[fix], toward[fix])
    return s.astype(F32)


def unpack_codes(codes, M, nbits):
    """[n, code_size] uint8 -> [n, M] indexes (PQDecoderGeneric)."""
    codes = np.asarray(codes, np.uint8)
    n = codes.shape[0]
    wide = np.zeros((n, codes.shape[1] + 1), np.uint32)
    wide[:, :-1] = codes
    out = np.empty((n, M), np.int64)
    for m in range(M):
        o = m * nbits
        v = wide[:, o >> 3] | (wide[:, (o >> 3) + 1] << 8)
        out[:, m] = (v >> (o & 7)) & ((1 << nbits) - 1)
    return out


def pack_codes(idx, nbits):
    """[n, M] indexes -> [n, (M nbits + 7) // 8] uint8 (PQEncoderGeneric)."""
    idx = np.asarray(idx, np.uint32)
    n, M = idx.shape
    cs = (M * nbits + 7) // 8
    out = np.zeros((n, cs + 1), np.uint32)
    for m in range(M):
        o = m * nbits
        v = idx[:, m] << (o & 7)
        out[:, o >> 3] |= v & 0xFF
        out[:, (o >> 3) + 1] |= v >> 8
    assert not out[:, cs].any()
    return out[:, :cs].astype(np.uint8)


def _term(x, y, l2):
    if l2:
        t = (x - y).astype(F32)
        return (t * t).astype(F32)
    return (x * y).astype(F32)


def _term_fma(x, y, acc, l2):
    if l2:
        t = (x - y).astype(F32)
        return fma(t, t, acc)
    return fma(x, y, acc)


def ny_entry(x, C, l2):
    """x [dsub], C [..., dsub] -> [...]: fvec_{L2sqr,inner_products}_ny, dsub 1/2/4/8."""
    dsub = C.shape[-1]
    assert dsub in (1, 2, 4, 8), "the model covers dsub 1, 2, 4 and 8"
    acc = _term(x[0], C[..., 0], l2)
    for j in range(1, dsub):
        acc = _term_fma(x[j], C[..., j], acc, l2)
    return acc


def ref_dist(x, Y, l2):
    """fvec_L2sqr / fvec_inner_product order (csrc/ref_arith.h): x [d], Y [..., d]."""
    d = Y.shape[-1]
    n8 = d & ~7
    c = [np.zeros(Y.shape[:-1], F32) for _ in range(8)]
    for i in range(0, n8, 8):
        for j in range(8):
            c[j] = _term_fma(x[i + j], Y[..., i + j], c[j], l2)
    r = (((c[0] + c[4]) + (c[2] + c[6])) + ((c[1] + c[5]) + (c[3] + c[7]))).astype(F32)
    i = n8
    if d - n8 >= 4:
        e = [_term(x[i + j], Y[..., i + j], l2) for j in range(4)]
        r = (r + ((e[0] + e[2]) + (e[1] + e[3]))).astype(F32)
        i += 4
    for j in range(i, d):
        r = _term_fma(x[j], Y[..., j], r, l2)
    return r


def heap_topk(arrivals, k, l2):
    """The reference's result heap over (distance, id) pairs in arrival order:
    a row is admitted when its distance strictly beats the heap's top (FLT_MAX /
    -FLT_MAX while the heap is not full), the worst (distance, id) pair is
    evicted, and the pairs come out best first, padded with -1 and +-FLT_MAX.
    Returns (D [k], I [k])."""
    D = np.full(k, FLT_MAX if l2 else -FLT_MAX, F32)
    I = np.full(k, -1, np.int64)
    heap = []  # best first; the last entry is the heap's top
    for dis, i in arrivals:
        key = (dis, i) if l2 else (-dis, -i)
        if len(heap) < k:
            if not (dis < FLT_MAX if l2 else dis > -FLT_MAX):
                continue
        elif key[0] < heap[-1][0]:  # strict admission on the distance alone
            heap.pop()
        else:
            continue
        bisect.insort(heap, key)
    for j, (a, b) in enumerate(heap):
        D[j], I[j] = (a, b) if l2 else (-a, -b)
    return D, I


class Model:
    """An IVF-PQ index as arrays: coarse centroids [nlist, d], PQ centroids
    [M, ksub, dsub], per list its packed codes [len, code_size] and ids."""

    def __init__(self, centroids, pq_centroids, nbits, list_codes, list_ids, metric_l2=True,
                 by_residual=True, table=1):
        self.cent = np.ascontiguousarray(centroids, F32)
        self.pqc = np.ascontiguousarray(pq_centroids, F32)
        self.M, self.ksub, self.dsub = self.pqc.shape
        self.nbits = int(nbits)
        assert self.ksub == 1 << self.nbits
        self.l2 = bool(metric_l2)
        self.by_residual = bool(by_residual)
        self.table1 = self.l2 and self.by_residual and table == 1
        self.idx = [unpack_codes(c, self.M, self.nbits) for c in list_codes]
        self.ids = [np.asarray(i, np.int64) for i in list_ids]
        if self.table1:  # the part of table 1 that depends on the list only
            self.cnorm = np.stack([ref_dist_self(self.pqc[m]) for m in range(self.M)])

    @classmethod
    def from_index(cls, idx, table=None):
        """From this library's IndexIVFPQ (host side only)."""
        info = idx.pq_info()
        nl = idx.nlist
        return cls(idx.quantizer.xb, idx.pq_centroids, info["nbits"],
                   [idx.list_codes(l) for l in range(nl)], [idx.list_ids(l) for l in range(nl)],
                   metric_l2=idx.metric_type == 1, by_residual=info["by_residual"],
                   table=info["use_precomputed_table"] if table is None else table)

    def tables(self, x, l, cd):
        """(dis0, tab [M, ksub]) of query x for list l (coarse distance cd)."""
        x = np.asarray(x, F32)
        yc = self.cent[l]
        M, ds = self.M, self.dsub
        tab = np.empty((M, self.ksub), F32)
        dis0 = F32(0)
        if not self.l2 or not self.by_residual:
            for m in range(M):
                tab[m] = ny_entry(x[m * ds:(m + 1) * ds], self.pqc[m], self.l2)
            if self.by_residual:  # inner product by residual: <x, y_C>
                dis0 = F32(ref_dist(x, yc[None, :], False)[0])
        elif self.table1:
            for m in range(M):
                sl = slice(m * ds, (m + 1) * ds)
                P = fma(F32(2), ny_entry(yc[sl], self.pqc[m], False), self.cnorm[m])
                tab[m] = fma(F32(-2), ny_entry(x[sl], self.pqc[m], False), P)
            dis0 = F32(cd)
        else:
            r = (x - yc).astype(F32)
            for m in range(M):
                tab[m] = ny_entry(r[m * ds:(m + 1) * ds], self.pqc[m], True)
        return dis0, tab

    def list_distances(self, x, l, cd):
        dis0, tab = self.tables(x, l, cd)
        idx = self.idx[l]
        r = np.zeros(idx.shape[0], F32)
        for m in range(self.M):  # the sequential sum
            r = (r + tab[m, idx[:, m]]).astype(F32)
        return (dis0 + r).astype(F32)

    def arrivals(self, x, keys, cdis, sel=None, max_codes=0):
        """(distance, id) of every scanned row of one query, in arrival order
        (max_codes as IndexIVF::search_preassigned's scan_one_list; sel: a set
        of admitted ids)."""
        nscan = 0
        for p, l in enumerate(keys):
            l = int(l)
            if l < 0 or len(self.ids[l]) == 0:
                continue
            n = len(self.ids[l])
            if max_codes:
                n = min(n, max_codes - nscan)
            dis = self.list_distances(x, l, cdis[p] if cdis is not None else 0.0)
            for j in range(n):
                if sel is None or int(self.ids[l][j]) in sel:
                    yield dis[j], int(self.ids[l][j])
            nscan += n
            if max_codes and nscan >= max_codes:
                break

    def search_preassigned(self, xq, k, keys, cdis, sel=None, max_codes=0):
        nq = len(xq)
        D = np.empty((nq, k), F32)
        I = np.empty((nq, k), np.int64)
        for q in range(nq):
            cd = cdis[q] if cdis is not None else None
            D[q], I[q] = heap_topk(self.arrivals(xq[q], keys[q], cd, sel, max_codes), k, self.l2)
        return D, I

    def range_search_preassigned(self, xq, radius, keys, cdis):
        lims, D, I = [0], [], []
        radius = F32(radius)
        for q in range(len(xq)):
            cd = cdis[q] if cdis is not None else None
            for dis, i in self.arrivals(xq[q], keys[q], cd):
                if dis < radius if self.l2 else dis > radius:
                    D.append(dis)
                    I.append(i)
            lims.append(len(D))
        return np.array(lims, np.int64), np.array(D, F32), np.array(I, np.int64)


def ref_dist_self(C):
    """|c|^2 of every row of C [ksub, dsub] in fvec_norm_L2sqr order."""
    out = np.empty(C.shape[0], F32)
    for j in range(C.shape[0]):
        out[j] = ref_dist(C[j], C[j][None, :], False)[0]
    return out
