"""Plain numpy model of the binary indexes' results (DESIGN.md §4 "Binary
indexes"): Hamming distances by unpackbits, and the three result rules of the
reference — flat, IVF with use_heap, IVF without.  Pads are (INT32_MAX, -1)."""
import numpy as np

PAD_D = np.iinfo(np.int32).max


def hamming(xq, xb):
    """[nq][nb] int32 distances between uint8 code rows."""
    x = np.asarray(xq, np.uint8)[:, None, :] ^ np.asarray(xb, np.uint8)[None, :, :]
    return np.unpackbits(x, axis=2).sum(axis=2).astype(np.int32)


def _emit(dis, ids, order, k):
    D = np.full(k, PAD_D, np.int32)
    I = np.full(k, -1, np.int64)
    order = order[:k]
    D[:len(order)] = dis[order]
    I[:len(order)] = ids[order]
    return D, I


def topk_sorted(dis, ids, k):
    """The k smallest by (distance, id), sorted that way (both flat scans)."""
    return _emit(dis, ids, np.lexsort((ids, dis)), k)


def topk_count(dis, ids, k):
    """Rows in arrival order: the k smallest by (distance, arrival), in that
    order (the counting scan)."""
    return _emit(dis, ids, np.argsort(dis, kind="stable"), k)


def topk_heap(dis, ids, k):
    """Rows in arrival order through the reference heap: strict admission,
    eviction of the largest (distance, id), output sorted by (distance, id)."""
    if len(dis) <= k:
        return topk_sorted(dis, ids, k)
    T = np.sort(dis, kind="stable")[k - 1]
    lt = np.flatnonzero(dis < T)
    first = np.flatnonzero(dis <= T)[:k]          # the first k arrivals with distance <= T
    A = first[dis[first] == T]                    # the tie rows that were admitted
    A = A[np.argsort(ids[A], kind="stable")][:k - len(lt)]
    keep = np.concatenate([lt, A])
    return _emit(dis, ids, keep[np.lexsort((ids[keep], dis[keep]))], k)


def flat_search(xb, xq, k):
    dis = hamming(xq, xb)
    ids = np.arange(len(xb), dtype=np.int64)
    out = [topk_sorted(row, ids, k) for row in dis]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


class IVFModel:
    """IndexBinaryIVF over given centroids: rows go to the nearest centroid
    (smallest (distance, list)), each list in add order."""

    def __init__(self, cent, xb, ids):
        self.cent, self.xb = np.asarray(cent, np.uint8), np.asarray(xb, np.uint8)
        self.ids = np.asarray(ids, np.int64)
        near = hamming(self.xb, self.cent).argmin(axis=1) if len(self.xb) else np.zeros(0, int)
        self.lists = [np.flatnonzero(near == l) for l in range(len(self.cent))]

    def probes(self, q, nprobe, max_codes=0):
        """Lists scanned for query row q, in coarse order."""
        nlist = len(self.cent)
        _, P = topk_sorted(hamming(q[None], self.cent)[0], np.arange(nlist, dtype=np.int64),
                           min(nprobe, nlist))
        out, nscan = [], 0
        for l in P:
            out.append(int(l))
            nscan += len(self.lists[l])
            if max_codes and nscan >= max_codes:
                break
        return out

    def arrivals(self, q, nprobe, max_codes=0):
        """Rows of xb in arrival order: (probe rank, offset in list)."""
        rows = [self.lists[l] for l in self.probes(q, nprobe, max_codes)]
        return np.concatenate(rows) if rows else np.zeros(0, int)

    def search(self, xq, k, nprobe, use_heap=True, max_codes=0):
        rule = topk_heap if use_heap else topk_count
        D, I = [], []
        for q in np.asarray(xq, np.uint8):
            rows = self.arrivals(q, nprobe, max_codes)
            d, i = rule(hamming(q[None], self.xb[rows])[0], self.ids[rows], k)
            D.append(d)
            I.append(i)
        return np.stack(D), np.stack(I)
