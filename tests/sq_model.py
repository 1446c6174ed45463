"""numpy restatement of the reference's IVF scalar-quantizer search (QT_8bit,
QT_fp16, d % 8 == 0), the rule csrc/sq_ref.h and csrc/kernels_sq.hip state in HIP.

* decode (Codec8bit::decode_8_components, QuantizerTemplate<.., NON_UNIFORM, 8>):
  xi = fma(float(code), 1/255, 0.5/255), x^ = fma(xi, vdiff, vmin) with
  vmin = trained[0..d), vdiff = trained[d..2d); fp16 is an exact widening.
* distance (SimilarityL2<8> / SimilarityIP<8>): lane j & 7 takes component j;
  L2 is t = y - x^ rounded, acc = fma(t, t, acc); inner product is
  acc = fma(y, x^, acc); the result is (s0 + s2) + (s1 + s3) with
  s_i = acc_i + acc_{i+4}.
* query side (IVFSQScannerL2 / IVFSQScannerIP::set_list): y = x - centroid, one
  rounded subtract per component, for L2 by residual, otherwise y = x; inner
  product by residual returns accu0 + s with accu0 the coarse distance.
* encode (encode_vector, Codec8bit::encode_component): the residual
  x - centroid when by residual (either metric); xi = (x - vmin) / vdiff
  clamped to [0, 1], 0 when vdiff == 0, code = int(255 xi); fp16 rounds to
  nearest even (values beyond 65504 become +-inf, NaN stays NaN).  A NaN input
  to the 8-bit encode is outside the model: the C++ conversion is undefined.
* search_preassigned (IndexIVF::search_preassigned): rows arrive probe by
  probe in list order; probes < 0 and empty lists are passed over; max_codes
  cuts the list that crosses it; a selector drops rows by id; store_pairs
  labels a row list << 32 | offset.  The result heap is
  pq_nbits_model.heap_topk.

fp32 throughout; fma() is the correctly rounded one of pq_nbits_model."""
import numpy as np

from pq_nbits_model import F32, FLT_MAX, fma, heap_topk  # noqa: F401

QT_8bit, QT_fp16 = 0, 4
_INV255 = F32(1) / F32(255)
_HALF255 = F32(0.5) / F32(255)


def decode(codes, qtype, trained, d):
    """[n, code_size] uint8 -> [n, d] float32 reconstructions."""
    codes = np.ascontiguousarray(codes, np.uint8)
    if qtype == QT_fp16:
        return codes.view("<f2").astype(F32).reshape(codes.shape[0], d)
    xi = fma(codes.astype(F32), _INV255, _HALF255)
    return fma(xi, trained[d:], trained[:d])


def encode(x, qtype, trained, d):
    """[n, d] float32 (residuals when by residual) -> [n, code_size] uint8."""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(all="ignore"):
        if qtype == QT_fp16:
            return np.ascontiguousarray(x.astype("<f2")).view(np.uint8).reshape(x.shape[0], 2 * d)
        vmin, vdiff = trained[:d], trained[d:]
        assert not np.isnan(x).any(), "NaN into the 8-bit encode is undefined in the reference"
        xi = ((x - vmin).astype(F32) / vdiff).astype(F32)
        xi = np.where(xi < 0, F32(0), xi)
        xi = np.where(xi > 1, F32(1), xi)
        xi = np.where(vdiff != 0, xi, F32(0)).astype(F32)
        return (F32(255) * xi).astype(F32).astype(np.int32).astype(np.uint8)


def distances(y, xr, l2):
    """y [nq, d] against xr [n, d] -> [nq, n], eight lane accumulators."""
    nq, d = y.shape
    assert d % 8 == 0
    acc = np.zeros((nq, xr.shape[0], 8), F32)
    with np.errstate(all="ignore"):
        for j in range(0, d, 8):
            yb, xb = y[:, None, j:j + 8], xr[None, :, j:j + 8]
            if l2:
                t = (yb - xb).astype(F32)
                acc = fma(t, t, acc)
            else:
                acc = fma(yb, xb, acc)
        s = (acc[..., :4] + acc[..., 4:]).astype(F32)
        s02 = (s[..., 0] + s[..., 2]).astype(F32)
        s13 = (s[..., 1] + s[..., 3]).astype(F32)
        return (s02 + s13).astype(F32)


class Model:
    """An IVF-SQ index as arrays: coarse centroids [nlist, d], trained
    (vmin | vdiff, empty for fp16), per list its codes [len, code_size] and ids."""

    def __init__(self, centroids, trained, qtype, list_codes, list_ids, metric_l2=True,
                 by_residual=True):
        self.cent = np.ascontiguousarray(centroids, F32)
        self.nlist, self.d = self.cent.shape
        self.qtype = int(qtype)
        assert self.qtype in (QT_8bit, QT_fp16) and self.d % 8 == 0
        self.trained = np.ascontiguousarray(trained, F32)
        assert self.trained.size == (2 * self.d if self.qtype == QT_8bit else 0)
        self.l2 = bool(metric_l2)
        self.by_residual = bool(by_residual)
        self.codes = [np.ascontiguousarray(c, np.uint8) for c in list_codes]
        self.ids = [np.asarray(i, np.int64) for i in list_ids]
        self.xr = [decode(c, self.qtype, self.trained, self.d) for c in self.codes]

    @classmethod
    def from_index(cls, idx):
        """From this library's IndexIVFScalarQuantizer (host side only)."""
        q = idx.quantizer
        cent = q.storage_vectors() if hasattr(q, "storage_vectors") else q.xb
        nl = idx.nlist
        return cls(cent, idx.sq_trained(), idx.qtype, [idx.list_codes(l) for l in range(nl)],
                   [idx.list_ids(l) for l in range(nl)], metric_l2=idx.metric_type == 1,
                   by_residual=idx.by_residual)

    def encode(self, x, lists):
        """The codes add_core stores for rows x sent to `lists`."""
        x = np.ascontiguousarray(x, F32)
        if self.by_residual:
            x = (x - self.cent[np.asarray(lists, np.int64)]).astype(F32)
        return encode(x, self.qtype, self.trained, self.d)

    def list_distances(self, xq, l, cd=None):
        """xq [nq, d] against every row of list l (cd [nq]: its coarse distances)."""
        xq = np.ascontiguousarray(xq, F32)
        y = (xq - self.cent[l]).astype(F32) if self.l2 and self.by_residual else xq
        s = distances(y, self.xr[l], self.l2)
        if not self.l2 and self.by_residual and cd is not None:
            with np.errstate(all="ignore"):
                s = (np.asarray(cd, F32)[:, None] + s).astype(F32)
        return s

    def arrivals(self, x, keys, cdis, sel=None, max_codes=0, store_pairs=False, dist=None):
        """(distance, label) of every scanned row of one query, in arrival order
        (dist(l, cd): the distances of list l, computed here when not given)."""
        if dist is None:
            def dist(l, cd):
                return self.list_distances(x[None, :], l, None if cd is None else [cd])[0]
        nscan = 0
        for p, l in enumerate(keys):
            l = int(l)
            if l < 0 or len(self.ids[l]) == 0:
                continue
            n = len(self.ids[l])
            if max_codes:
                n = min(n, max_codes - nscan)
            dis = dist(l, None if cdis is None else cdis[p]).tolist()  # fp32 values, exact
            ids = self.ids[l].tolist()
            for j in range(n):
                if sel is None or ids[j] in sel:
                    yield dis[j], (l << 32 | j) if store_pairs else ids[j]
            nscan += n
            if max_codes and nscan >= max_codes:
                break

    def search_preassigned(self, xq, k, keys, cdis, sel=None, max_codes=0, store_pairs=False):
        xq = np.ascontiguousarray(xq, F32)
        keys = np.asarray(keys, np.int64)
        nq = len(xq)
        # every probed list once, against all the queries that name it
        base = {}
        for l in np.unique(keys[keys >= 0]).tolist():
            if len(self.ids[l]):
                qs = np.nonzero((keys == l).any(axis=1))[0]
                s = self.list_distances(xq[qs], l)
                base[l] = {int(q): s[r] for r, q in enumerate(qs)}
        add_cd = not self.l2 and self.by_residual and cdis is not None
        D = np.empty((nq, k), F32)
        I = np.empty((nq, k), np.int64)
        for q in range(nq):
            def dist(l, cd, q=q):
                with np.errstate(all="ignore"):
                    return (F32(cd) + base[l][q]).astype(F32) if add_cd else base[l][q]
            cd = cdis[q] if cdis is not None else None
            D[q], I[q] = heap_topk(
                self.arrivals(xq[q], keys[q], cd, sel, max_codes, store_pairs, dist), k, self.l2)
        return D, I
