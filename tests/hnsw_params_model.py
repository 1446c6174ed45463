"""A plain Python restatement of HNSW::search in its three level-0 modes
(faiss/impl/HNSW.cpp:943-996): the bounded MinimaxHeap search with the
relative-distance stop (the default), the same with check_relative_distance
false (stop after efSearch level-0 hops), and bounded_queue false
(search_from_candidate_unbounded, two priority queues of (distance, id)
pairs), with the selector that gates the result heap of the bounded forms.

Distances are oracle.fvec_L2sqr (the reference's evaluation order), the graph
comes from oracle.HNSWGraph.from_index.  tests/test_hnsw_params_model.py holds
this restatement to the reference-run fixtures bit for bit, stats included;
tests/test_gpu_hnsw_params.py then uses it for shapes that have no fixture.
"""
import heapq

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)


class MinimaxHeap:
    """HNSW::MinimaxHeap (:1096-1342) over faiss's binary max-heap layout
    (heap_push / heap_pop of faiss/utils/Heap.h, CMax with cmp2), 1-based."""

    def __init__(self, n):
        self.n, self.k, self.nvalid = n, 0, 0
        self.dis = np.zeros(n + 2, np.float64)
        self.ids = np.zeros(n + 2, np.int64)

    @staticmethod
    def _gt(v1, i1, v2, i2):  # CMax::cmp2
        return v1 > v2 or (v1 == v2 and i1 > i2)

    def _heap_pop(self):
        k, dis, ids = self.k, self.dis, self.ids
        val, idv = dis[k], ids[k]
        i = 1
        while True:
            i1 = 2 * i
            i2 = i1 + 1
            if i1 > k:
                break
            if i2 == k + 1 or self._gt(dis[i1], ids[i1], dis[i2], ids[i2]):
                if self._gt(val, idv, dis[i1], ids[i1]):
                    break
                dis[i], ids[i] = dis[i1], ids[i1]
                i = i1
            else:
                if self._gt(val, idv, dis[i2], ids[i2]):
                    break
                dis[i], ids[i] = dis[i2], ids[i2]
                i = i2
        dis[i], ids[i] = dis[k], ids[k]
        self.k -= 1

    def _heap_push(self, val, idv):
        self.k += 1
        dis, ids = self.dis, self.ids
        i = self.k
        while i > 1:
            f = i >> 1
            if not self._gt(val, idv, dis[f], ids[f]):
                break
            dis[i], ids[i] = dis[f], ids[f]
            i = f
        dis[i], ids[i] = val, idv

    def push(self, i, v):
        if self.k == self.n:
            if v >= self.dis[1]:
                return
            if self.ids[1] != -1:
                self.nvalid -= 1
            self._heap_pop()
        self._heap_push(v, i)
        self.nvalid += 1

    def pop_min(self):
        """(id, dis) of the smallest live entry, the highest slot among equal
        minima; the slot keeps its distance with id -1."""
        k = self.k
        live = self.ids[1:k + 1] != -1
        if not live.any():
            return -1, 0.0
        d = np.where(live, self.dis[1:k + 1], np.inf)
        imin = k - int(np.argmin(d[::-1]))
        ret = int(self.ids[imin])
        self.ids[imin] = -1
        self.nvalid -= 1
        return ret, float(self.dis[imin])

    def count_below(self, thresh):
        return int((self.dis[1:self.k + 1] < thresh).sum())


class Model:
    def __init__(self, orc, graph):
        self.orc, self.g = orc, graph
        self.ntotal = graph.storage.shape[0]
        self.nb0 = int(graph.cum[1] - graph.cum[0]) if len(graph.cum) > 1 else 0
        self.queue_high_water = 0  # largest `candidates` size of any Mode B query
        self._dis = {}  # query bytes -> {node: distance}, shared by the searches

    def _neighbors(self, v, level):
        g = self.g
        o = int(g.offsets[v])
        out = []
        for j in range(o + int(g.cum[level]), o + int(g.cum[level + 1])):
            w = int(g.neighbors[j])
            if w < 0:
                break
            out.append(w)
        return out

    def search(self, xq, k, efSearch, check_relative_distance=True, bounded_queue=True,
               member=None):
        """D, I (int64) and the HNSWStats deltas [n1, n2, ndis, nhops]; member:
        bool per node (None: every node)."""
        xq = np.ascontiguousarray(xq, np.float32)
        nq = xq.shape[0]
        D = np.full((nq, k), FLT_MAX, np.float32)
        I = np.full((nq, k), -1, np.int64)
        st = np.zeros(4, np.int64)
        for qi in range(nq):
            res = self._one(xq[qi], k, efSearch, check_relative_distance, bounded_queue,
                            member, st)
            for j, (d, i) in enumerate(res):
                D[qi, j], I[qi, j] = d, i
        return D, I, st

    def _one(self, q, k, efSearch, check, bounded, member, st):
        g = self.g
        if self.ntotal == 0 or g.s.entry_point < 0:
            return []
        cache = self._dis.setdefault(q.tobytes(), {})

        def dis(v):
            r = cache.get(v)
            if r is None:
                r = cache[v] = float(self.orc.fvec_L2sqr(q, g.storage[v]))
            return r

        # greedy_update_nearest on the upper levels (:852-924)
        nearest = int(g.s.entry_point)
        d_nearest = dis(nearest)
        for level in range(int(g.s.max_level), 0, -1):
            while True:
                prev = nearest
                nb = self._neighbors(nearest, level)
                for v in nb:
                    dv = dis(v)
                    if dv < d_nearest:
                        nearest, d_nearest = v, dv
                st[2] += len(nb)
                st[3] += 1
                if nearest == prev:
                    break
        ef = max(efSearch, k)
        visited = {nearest}
        if not bounded:
            return self._unbounded(nearest, d_nearest, dis, visited, ef, k, st)
        # search_from_candidates (:605-741); the result heap as a set: its top
        # is the largest (dis, id), add_result replaces it when dis < top's dis
        res = [(-float(FLT_MAX), 1)] * k  # heapq of (-dis, -id): (FLT_MAX, -1) k times

        def add_result(d, v):
            if (member is None or member[v]) and d < -res[0][0]:
                heapq.heapreplace(res, (-d, -v))

        cand = MinimaxHeap(ef)
        cand.push(nearest, d_nearest)
        add_result(d_nearest, nearest)
        nstep = ndis = 0
        while cand.nvalid > 0:
            v0, d0 = cand.pop_min()
            if check and cand.count_below(d0) >= efSearch:
                break
            for v in self._neighbors(v0, 0):
                if v in visited:
                    continue
                visited.add(v)
                dv = dis(v)
                ndis += 1
                add_result(dv, v)
                cand.push(v, dv)
            nstep += 1
            if not check and nstep > efSearch:
                break
        st[0] += 1
        st[1] += 1 if cand.nvalid == 0 else 0
        st[2] += ndis
        st[3] += nstep
        return sorted((np.float32(-d), -i) for d, i in res if -i != -1)

    def _unbounded(self, nearest, d_nearest, dis, visited, ef, k, st):
        top = [(-d_nearest, -nearest)]  # max-queue of (dis, id), at most ef entries
        cand = [(d_nearest, nearest)]   # min-queue, no bound
        ndis = 0
        while cand:
            d0, v0 = cand[0]
            if d0 > -top[0][0]:
                break
            heapq.heappop(cand)
            for v in self._neighbors(v0, 0):
                if v in visited:
                    continue
                visited.add(v)
                dv = dis(v)
                ndis += 1
                if -top[0][0] > dv or len(top) < ef:
                    heapq.heappush(cand, (dv, v))
                    heapq.heappush(top, (-dv, -v))
                    if len(top) > ef:
                        heapq.heappop(top)
                    self.queue_high_water = max(self.queue_high_water, len(cand))
            st[3] += 1
        st[0] += 1
        st[1] += 1 if not cand else 0
        st[2] += ndis
        return [(np.float32(d), i) for d, i in sorted((-d, -i) for d, i in top)[:k]]
