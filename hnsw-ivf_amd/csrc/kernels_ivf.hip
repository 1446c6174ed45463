// kernels_ivf.hip — list-centric batched IVF-Flat scan for gfx950.
//
// Reference hot loop: faiss/IndexIVFFlat.cpp:155-179 (IVFFlatScanner::
// scan_codes: for each code, dis = fvec_L2sqr(x, y, d); heap_replace_top on
// strict improvement) driven per query by faiss/IndexIVF.cpp:595-631.
//
// MI355X design: instead of streaming every probed list once per query (the
// CPU order, ~4 MB/query at nlist 4096 nprobe 32), the (query, list) pairs of
// the whole batch are bucketed by list.  A workgroup owns one list and up to
// 64 of the queries probing it: the list is read from HBM once per 64 queries,
// tiles of 64 queries x 64 codes live in LDS, and each thread computes a 4x4
// micro-tile of exact sum (x-y)^2 (same arithmetic as the reference, not the
// norm expansion).  Each wave then folds its 16 queries' distance rows into
// wave64 top-k queues and the per-(query, list) top-k is written out; a
// second kernel merges the nprobe partial lists of each query.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include <algorithm>

#include <cfloat>

#include "common.h"
#include "kernels.h"
#include "ref_arith.h"
#include "wave_select.h"

namespace faiss_amd {
namespace kern {

// ---------------------------------------------------------------- bucketing
// counts per list; the value returned by the atomic is the entry's slot in
// its bucket, so the fill needs no second round of atomics
__global__ void k_bucket_count(const int32_t* __restrict__ assign, int64_t total,
                               const uint32_t* __restrict__ list_len, int nlist,
                               uint32_t* __restrict__ counts, uint32_t* __restrict__ pos) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int l = assign[e];
    if (l >= 0 && l < nlist && list_len[l] > 0) pos[e] = atomicAdd(&counts[l], 1u);
}

// Same with a block-local LDS histogram (nlist <= BC_MAXL): BC_PER entries
// per thread take their slot from an LDS atomic, then one global atomic per
// non-empty bin reserves the block's range of each bucket.
constexpr int BC_MAXL = 16384;       // lists per range in 64 KB of LDS
constexpr int BC_MAXL_BIG = 32768;   // 128 KB (a work group may hold 160 KB on gfx950)
template <int BC_PER>
__global__ __launch_bounds__(1024) void k_bucket_count_lds(const int32_t* __restrict__ assign,
                                                           int64_t total,
                                                           const uint32_t* __restrict__ list_len,
                                                           int nlist, uint32_t* __restrict__ counts,
                                                           uint32_t* __restrict__ pos, int maxl) {
    extern __shared__ uint32_t hist[];  // [min(nlist, maxl)]
    const int t = threadIdx.x;
    // lists [lbase, lbase + nl) of this block row (nlist > maxl: one row of
    // blocks per range, each reading every entry)
    const int lbase = (int)blockIdx.y * maxl;
    const int nl = min(maxl, nlist - lbase);
    for (int i = t; i < nl; i += 1024) hist[i] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * 1024 * BC_PER;
    int ll[BC_PER];
    uint32_t lp[BC_PER];
#pragma unroll
    for (int j = 0; j < BC_PER; j++) {
        const int64_t e = base + (int64_t)j * 1024 + t;
        int l = -1;
        if (e < total) {
            l = assign[e];
            if (!(l >= 0 && l < nlist && list_len[l] > 0)) l = -1;
        }
        l = (l >= lbase && l < lbase + nl) ? l - lbase : -1;
        ll[j] = l;
        lp[j] = l >= 0 ? atomicAdd(&hist[l], 1u) : 0u;
    }
    __syncthreads();
    for (int i = t; i < nl; i += 1024) {
        const uint32_t c = hist[i];
        if (c) hist[i] = atomicAdd(&counts[lbase + i], c);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BC_PER; j++) {
        const int64_t e = base + (int64_t)j * 1024 + t;
        if (ll[j] >= 0) pos[e] = hist[ll[j]] + lp[j];
    }
}

// single-workgroup exclusive scan of counts -> bucket_off, ceil(counts/QT)
// -> item_off; per work item its list when asked.  E consecutive counts per
// thread (E = nlist / 1024 rounded up to a power of two, at most 64): every
// count of a chunk of 1024 E lists is loaded at once (one round trip — c5's
// 65536 lists in one chunk instead of sixteen), thread sums, shuffle scan per
// wave, 16 wave totals through LDS; a running carry between chunks.
template <int E>
__global__ __launch_bounds__(1024) void k_bucket_scan(const uint32_t* counts,
                                                      int nlist, int QT,
                                                      uint32_t* __restrict__ bucket_off,
                                                      uint32_t* __restrict__ item_off,
                                                      uint32_t* __restrict__ item_list,
                                                      uint32_t* zero_next,
                                                      uint32_t* __restrict__ item_ctr,
                                                      const uint32_t* __restrict__ perm) {
    __shared__ uint32_t wb[16], wi[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    constexpr int CH = 1024 * E;
    static_assert(E % 4 == 0, "E counts per thread as uint4 groups");
    // items of a bucket of c entries: ceil(c / QT), a shift when QT is a power
    // of two (every caller's), else a division
    const int qs = (QT & (QT - 1)) == 0 ? __builtin_ctz((unsigned)QT) : -1;
    auto nitems = [&](uint32_t c) -> uint32_t {
        return qs >= 0 ? (c + (uint32_t)QT - 1u) >> qs : (c + (uint32_t)QT - 1u) / (uint32_t)QT;
    };
    // prefix of the thread sums (v[] per thread) over the work group: returns
    // this thread's exclusive prefix and the chunk total
    auto block_scan = [&](uint32_t sb, uint32_t si, uint32_t& pb, uint32_t& pi, uint32_t& tb,
                          uint32_t& ti) {
        uint32_t ib = sb, ii = si;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t vb = __shfl_up(ib, off), vi = __shfl_up(ii, off);
            if (lane >= off) {
                ib += vb;
                ii += vi;
            }
        }
        if (lane == 63) {
            wb[w] = ib;
            wi[w] = ii;
        }
        __syncthreads();
        pb = 0;
        pi = 0;
        tb = 0;
        ti = 0;
#pragma unroll
        for (int v = 0; v < 16; v++) {
            pb += v < w ? wb[v] : 0u;
            pi += v < w ? wi[v] : 0u;
            tb += wb[v];
            ti += wi[v];
        }
        __syncthreads();  // wb / wi are rewritten by the next chunk
        pb += ib - sb;
        pi += ii - si;
    };
    uint32_t carry_b = 0, carry_i = 0;
    for (int c0 = 0; c0 < nlist; c0 += CH) {
        const int l0 = c0 + E * t;
        uint32_t c[E];
        uint32_t sb = 0, si = 0;
        const bool full = l0 + E <= nlist;  // this thread's E lists exist (uint4 access)
        if (full) {
#pragma unroll
            for (int v = 0; v < E / 4; v++) {
                const uint4 c4 = *(const uint4*)(counts + l0 + 4 * v);
                c[4 * v] = c4.x;
                c[4 * v + 1] = c4.y;
                c[4 * v + 2] = c4.z;
                c[4 * v + 3] = c4.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < E; j++) c[j] = l0 + j < nlist ? counts[l0 + j] : 0u;
        }
        // zero_next == counts: each count is cleared once read (the fill
        // takes the bucket sizes from bucket_off)
        if (zero_next) {
            if (full) {
#pragma unroll
                for (int v = 0; v < E / 4; v++)
                    *(uint4*)(zero_next + l0 + 4 * v) = make_uint4(0u, 0u, 0u, 0u);
            } else {
                for (int j = 0; j < E && l0 + j < nlist; j++) zero_next[l0 + j] = 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < E; j++) {
            sb += c[j];
            si += nitems(c[j]);
        }
        uint32_t pb, pi, tb, ti;
        block_scan(sb, si, pb, pi, tb, ti);
        uint32_t rb = carry_b + pb, ri = carry_i + pi;  // exclusive prefix of this thread
        uint32_t ob[E], oi[E];
#pragma unroll
        for (int j = 0; j < E; j++) {
            ob[j] = rb;
            oi[j] = ri;
            rb += c[j];
            ri += nitems(c[j]);
        }
        if (full) {
#pragma unroll
            for (int v = 0; v < E / 4; v++) {
                *(uint4*)(bucket_off + l0 + 4 * v) =
                        make_uint4(ob[4 * v], ob[4 * v + 1], ob[4 * v + 2], ob[4 * v + 3]);
                *(uint4*)(item_off + l0 + 4 * v) =
                        make_uint4(oi[4 * v], oi[4 * v + 1], oi[4 * v + 2], oi[4 * v + 3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < E; j++) {
                if (l0 + j < nlist) {
                    bucket_off[l0 + j] = ob[j];
                    item_off[l0 + j] = oi[j];
                }
            }
        }
        if (item_list) {  // rare (item_list users); a second walk keeps the first lean
            ri = carry_i + pi;
            for (int j = 0; j < E && l0 + j < nlist; j++) {
                const uint32_t nj = nitems(c[j]);
                for (uint32_t i = 0; i < nj; i++) item_list[ri + i] = (uint32_t)(l0 + j);
                ri += nj;
            }
        }
        carry_b += tb;
        carry_i += ti;
    }
    if (t == 0) {
        bucket_off[nlist] = carry_b;
        item_off[nlist] = carry_i;
        if (item_ctr) *item_ctr = 0u;  // the persistent filter's work counter
    }
    if (!perm) return;
    // items renumbered in perm order (bucket sizes from bucket_off: the counts
    // are cleared); the bucket_off stores above are this work group's own
    __threadfence_block();
    __syncthreads();
    carry_i = 0;
    for (int c0 = 0; c0 < nlist; c0 += CH) {
        const int i0 = c0 + E * t;
        int ls[E];
        uint32_t n[E], si = 0;
        if (i0 + E <= nlist) {
#pragma unroll
            for (int v = 0; v < E / 4; v++) {
                const uint4 p4 = *(const uint4*)(perm + i0 + 4 * v);
                ls[4 * v] = (int)p4.x;
                ls[4 * v + 1] = (int)p4.y;
                ls[4 * v + 2] = (int)p4.z;
                ls[4 * v + 3] = (int)p4.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < E; j++) ls[j] = i0 + j < nlist ? (int)perm[i0 + j] : -1;
        }
#pragma unroll
        for (int j = 0; j < E; j++) {
            n[j] = ls[j] >= 0 ? nitems(bucket_off[ls[j] + 1] - bucket_off[ls[j]]) : 0u;
            si += n[j];
        }
        uint32_t pb, pi, tb, ti;
        block_scan(0u, si, pb, pi, tb, ti);
        uint32_t ri = carry_i + pi;
#pragma unroll
        for (int j = 0; j < E; j++) {
            if (ls[j] >= 0) item_off[ls[j]] = ri;
            ri += n[j];
        }
        if (item_list) {  // rare (item_list users); a second walk keeps the first lean
            ri = carry_i + pi;
            for (int j = 0; j < E; j++) {
                for (uint32_t i = 0; i < n[j]; i++) item_list[ri + i] = (uint32_t)ls[j];
                ri += n[j];
            }
        }
        carry_i += ti;
    }
}

// The scan of k_bucket_scan over many work groups (nlist > 8192; c5: 65536
// lists, where the single work group's chunks and its gathers of the
// permuted counts took 133 us).  Part: each group scans its 4096 E-runs of
// counts (bucket sizes, and work items in list order or, with perm, in perm
// order — the counts gathered through perm) into local exclusive prefixes
// and writes its three totals; fix: each group adds the totals of the groups
// before it, clears its counts (counts_next) and the last one writes the
// ends and the work counter.
template <int E>
__global__ __launch_bounds__(1024) void k_bucket_scan_part(const uint32_t* __restrict__ counts,
                                                           int nlist, int QT,
                                                           uint32_t* __restrict__ bucket_off,
                                                           uint32_t* __restrict__ item_off,
                                                           const uint32_t* __restrict__ perm,
                                                           uint32_t* __restrict__ tot) {
    __shared__ uint32_t wb[16], wi[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int qs = (QT & (QT - 1)) == 0 ? __builtin_ctz((unsigned)QT) : -1;
    auto nitems = [&](uint32_t c) -> uint32_t {
        return qs >= 0 ? (c + (uint32_t)QT - 1u) >> qs : (c + (uint32_t)QT - 1u) / (uint32_t)QT;
    };
    auto block_scan = [&](uint32_t sb, uint32_t si, uint32_t& pb, uint32_t& pi, uint32_t& tb,
                          uint32_t& ti) {
        uint32_t ib = sb, ii = si;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t vb = __shfl_up(ib, off), vi = __shfl_up(ii, off);
            if (lane >= off) {
                ib += vb;
                ii += vi;
            }
        }
        if (lane == 63) {
            wb[w] = ib;
            wi[w] = ii;
        }
        __syncthreads();
        pb = pi = tb = ti = 0u;
#pragma unroll
        for (int v = 0; v < 16; v++) {
            pb += v < w ? wb[v] : 0u;
            pi += v < w ? wi[v] : 0u;
            tb += wb[v];
            ti += wi[v];
        }
        __syncthreads();
        pb += ib - sb;
        pi += ii - si;
    };
    const int l0 = (int)blockIdx.x * 1024 * E + E * t;
    uint32_t c[E], sb = 0u, si = 0u;
#pragma unroll
    for (int j = 0; j < E; j++) {
        c[j] = l0 + j < nlist ? counts[l0 + j] : 0u;
        sb += c[j];
        si += nitems(c[j]);
    }
    uint32_t pb, pi, tb, ti;
    block_scan(sb, si, pb, pi, tb, ti);
#pragma unroll
    for (int j = 0; j < E; j++) {
        if (l0 + j < nlist) {
            bucket_off[l0 + j] = pb;
            if (!perm) item_off[l0 + j] = pi;
        }
        pb += c[j];
        pi += nitems(c[j]);
    }
    uint32_t tp = 0u;
    if (perm) {
        int ls[E];
        uint32_t nj[E], sp = 0u;
#pragma unroll
        for (int j = 0; j < E; j++) {
            ls[j] = l0 + j < nlist ? (int)perm[l0 + j] : -1;
            nj[j] = ls[j] >= 0 ? nitems(counts[ls[j]]) : 0u;
            sp += nj[j];
        }
        uint32_t pp, dummy, tdummy;
        block_scan(sp, 0u, pp, dummy, tp, tdummy);
#pragma unroll
        for (int j = 0; j < E; j++) {
            if (ls[j] >= 0) item_off[ls[j]] = pp;
            pp += nj[j];
        }
    }
    if (t == 0) {
        tot[3 * blockIdx.x] = tb;
        tot[3 * blockIdx.x + 1] = ti;
        tot[3 * blockIdx.x + 2] = tp;
    }
}
template <int E>
__global__ __launch_bounds__(1024) void k_bucket_scan_fix(int nlist, uint32_t* __restrict__ bucket_off,
                                                          uint32_t* __restrict__ item_off,
                                                          const uint32_t* __restrict__ perm,
                                                          const uint32_t* __restrict__ tot,
                                                          uint32_t* __restrict__ zero_next,
                                                          uint32_t* __restrict__ item_ctr) {
    const int t = threadIdx.x, b = (int)blockIdx.x;
    uint32_t ob = 0u, oi = 0u;
    for (int v = 0; v < b; v++) {
        ob += tot[3 * v];
        oi += tot[3 * v + (perm ? 2 : 1)];
    }
    const int l0 = b * 1024 * E + E * t;
#pragma unroll
    for (int j = 0; j < E; j++) {
        if (l0 + j < nlist) {
            bucket_off[l0 + j] += ob;
            item_off[perm ? (int)perm[l0 + j] : l0 + j] += oi;
            if (zero_next) zero_next[l0 + j] = 0u;
        }
    }
    if (b == (int)gridDim.x - 1 && t == 0) {
        bucket_off[nlist] = ob + tot[3 * b];
        item_off[nlist] = oi + tot[3 * b + (perm ? 2 : 1)];
        if (item_ctr) *item_ctr = 0u;
    }
}

__global__ void k_bucket_fill(const int32_t* __restrict__ assign, int64_t total,
                              const uint32_t* __restrict__ list_len, int nlist, int QT,
                              const uint32_t* __restrict__ bucket_off,
                              const uint32_t* __restrict__ item_off,
                              const uint32_t* __restrict__ pos, uint32_t* __restrict__ entries,
                              uint32_t* __restrict__ item_entries, ItemDesc* __restrict__ item_desc,
                              const uint32_t* __restrict__ counts,
                              const uint32_t* __restrict__ list_off,
                              uint32_t* __restrict__ mkeys, ProbeRec* __restrict__ mrecs,
                              int ke) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int l = assign[e];
    if (l >= 0 && l < nlist && list_len[l] > 0) {
        const uint32_t p = pos[e];
        if (item_entries) {
            const uint32_t item = item_off[l] + p / QT;
            item_entries[item * QT + p % QT] = (uint32_t)e;
            if (p % QT == 0) {  // the item's first entry writes its descriptor
                ItemDesc dsc;
                dsc.l = (uint32_t)l;
                dsc.nq = min((uint32_t)QT, bucket_off[l + 1] - bucket_off[l] - p);
                dsc.len = list_len[l];
                dsc.off = list_off[l];
                item_desc[item] = dsc;
            }
        } else {
            entries[bucket_off[l] + p] = (uint32_t)e;
        }
    } else if (mkeys) {
        for (int i = 0; i < ke; i++) mkeys[e * ke + i] = 0xffffffffu;
        ProbeRec pr;
        for (int i = 0; i < 4; i++) pr.pb[i] = WS_INF;
        pr.mmax = 0.f;
        pr.off = 0u;
        pr.len = 0u;
        pr.pad = 0u;
        mrecs[e] = pr;
    }
}

// ------------------------------------------------ the scan inside the fill
// Up to BF_MAXL lists (and no item_list) the prefix sums of k_bucket_scan are
// rebuilt in the LDS of every work group of the fill instead of by a launch
// of their own: the scan kernel was one work group's launch, drain and two
// dependent round trips on the critical path (c2: 8 us of a 270 us step) for
// a few KB of traffic.  k_bucket_fill_scan follows k_bucket_count_lds (two
// launches); k_bucket_one also builds the histogram, in one work group, for
// batches of at most BF_ONE_MAX entries (one launch; c1: 8000).
constexpr int BF_MAXL = 8192;           // E = 8 counts per thread, 4 x 32 KB of LDS
constexpr int64_t BF_ONE_MAX = 16384;   // 16 entries per thread of one work group

struct BFArgs {
    const int32_t* assign;
    int64_t total;
    const uint32_t* list_len;
    const uint32_t* list_off;
    int nlist, QT;
    uint32_t* bucket_off;
    uint32_t* item_off;
    uint32_t* item_ctr;
    const uint32_t* perm;
    uint32_t* entries;
    uint32_t* item_entries;
    ItemDesc* item_desc;
    uint32_t* mkeys;
    ProbeRec* mrecs;
    int ke;
};

// What k_bucket_scan computes, for one work group of 1024 threads with the
// counts in LDS (cnt, complete): c = this thread's counts of lists [E t,
// E t + E) (0 past nlist), ls = the lists at [E t, E t + E) of the item order
// (perm, or the identity; -1 past nlist).  off[l] becomes the first work item
// of list l (item_entries given) or the first slot of its bucket (entries);
// `global` also writes bucket_off, item_off and the work counter as the scan
// kernel does.  off[] is complete for every thread on return (a barrier).
template <int E>
__device__ __forceinline__ void bf_offsets(const BFArgs& a, const uint32_t* cnt, uint32_t* off,
                                           uint32_t* wb, uint32_t* wi, const uint32_t (&c)[E],
                                           const int (&ls)[E], int qs, bool global) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, l0 = E * t;
    const uint32_t QT = (uint32_t)a.QT;
    auto nitems = [&](uint32_t v) -> uint32_t {
        return qs >= 0 ? (v + QT - 1u) >> qs : (v + QT - 1u) / QT;
    };
    uint32_t n[E], sb = 0u, si = 0u;
#pragma unroll
    for (int j = 0; j < E; j++) {
        n[j] = ls[j] >= 0 ? nitems(cnt[ls[j]]) : 0u;
        sb += c[j];
        si += n[j];
    }
    uint32_t ib = sb, ii = si;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t vb = __shfl_up(ib, o), vi = __shfl_up(ii, o);
        if (lane >= o) {
            ib += vb;
            ii += vi;
        }
    }
    if (lane == 63) {
        wb[w] = ib;
        wi[w] = ii;
    }
    __syncthreads();
    uint32_t pb = ib - sb, pi = ii - si, tb = 0u, ti = 0u;
#pragma unroll
    for (int v = 0; v < 16; v++) {
        pb += v < w ? wb[v] : 0u;
        pi += v < w ? wi[v] : 0u;
        tb += wb[v];
        ti += wi[v];
    }
    uint32_t ob[E], oi[E];
#pragma unroll
    for (int j = 0; j < E; j++) {
        ob[j] = pb;
        oi[j] = pi;
        pb += c[j];
        pi += n[j];
    }
    if (a.item_entries) {
#pragma unroll
        for (int j = 0; j < E; j++)
            if (ls[j] >= 0) off[ls[j]] = oi[j];
    } else {
#pragma unroll
        for (int j = 0; j < E; j++)
            if (l0 + j < a.nlist) off[l0 + j] = ob[j];
    }
    if (global) {
        if (l0 + E <= a.nlist) {
#pragma unroll
            for (int v = 0; v < E / 4; v++)
                *(uint4*)(a.bucket_off + l0 + 4 * v) =
                        make_uint4(ob[4 * v], ob[4 * v + 1], ob[4 * v + 2], ob[4 * v + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < E; j++)
                if (l0 + j < a.nlist) a.bucket_off[l0 + j] = ob[j];
        }
        if (!a.item_entries) {
#pragma unroll
            for (int j = 0; j < E; j++)
                if (ls[j] >= 0) a.item_off[ls[j]] = oi[j];
        }
        if (t == 0) {
            a.bucket_off[a.nlist] = tb;
            a.item_off[a.nlist] = ti;
            if (a.item_ctr) *a.item_ctr = 0u;  // the persistent filter's work counter
        }
    }
    __syncthreads();
    if (global && a.item_entries) {  // off[] is item_off by list: copied out coalesced
        if (l0 + E <= a.nlist) {
#pragma unroll
            for (int v = 0; v < E / 4; v++)
                *(uint4*)(a.item_off + l0 + 4 * v) =
                        make_uint4(off[l0 + 4 * v], off[l0 + 4 * v + 1], off[l0 + 4 * v + 2],
                                   off[l0 + 4 * v + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < E; j++)
                if (l0 + j < a.nlist) a.item_off[l0 + j] = off[l0 + j];
        }
    }
}

// what k_bucket_fill stores for entry e of list l (-1: not a list) at slot p
// of its bucket; geo = the lists' {length, arena offset} in LDS.  A list that
// is probed by a valid entry has a count of at least one, and a list of
// length 0 has none, so cnt[l] > 0 stands for the fill's list_len[l] > 0.
__device__ __forceinline__ void bf_store(const BFArgs& a, const uint32_t* cnt, const uint32_t* off,
                                         const uint2* geo, int qs, int64_t e, int l, uint32_t p) {
    const uint32_t QT = (uint32_t)a.QT;
    const uint32_t c = l >= 0 ? cnt[l] : 0u;
    if (c) {
        if (a.item_entries) {
            const uint32_t pq = qs >= 0 ? p >> qs : p / QT, pr = p - pq * QT;
            const uint32_t item = off[l] + pq;
            a.item_entries[item * QT + pr] = (uint32_t)e;
            if (pr == 0) {  // the item's first entry writes its descriptor
                ItemDesc dsc;
                dsc.l = (uint32_t)l;
                dsc.nq = min(QT, c - p);
                const uint2 g = geo[l];
                dsc.len = g.x;
                dsc.off = g.y;
                a.item_desc[item] = dsc;
            }
        } else {
            a.entries[off[l] + p] = (uint32_t)e;
        }
    } else if (a.mkeys) {
        for (int i = 0; i < a.ke; i++) a.mkeys[e * a.ke + i] = 0xffffffffu;
        ProbeRec pr;
        for (int i = 0; i < 4; i++) pr.pb[i] = WS_INF;
        pr.mmax = 0.f;
        pr.off = 0u;
        pr.len = 0u;
        pr.pad = 0u;
        a.mrecs[e] = pr;
    }
}

// Words [E t, E t + E) of a per-list array, as uint4 groups and without a
// branch: a load under a branch is waited for where the branch ends, and the
// loads of these kernels are meant to be in flight together.  The arrays are
// allocated in whole uint4 groups (IVFBuckets), so the group that holds the
// last list may be read whole; a thread past it reads that group again, and
// the caller masks what lies past nlist.
template <int E>
__device__ __forceinline__ void bf_load_words(const uint32_t* p, int nlist, uint32_t (&v)[E]) {
    const int g0 = (E / 4) * (int)threadIdx.x, glast = (nlist + 3) / 4 - 1;
#pragma unroll
    for (int u = 0; u < E / 4; u++) {
        const uint4 x = ((const uint4*)p)[min(g0 + u, glast)];
        v[4 * u] = x.x;
        v[4 * u + 1] = x.y;
        v[4 * u + 2] = x.z;
        v[4 * u + 3] = x.w;
    }
}
// the lists at [E t, E t + E) of the item order from the words of perm (or
// of any array when there is no perm: the identity), -1 past nlist
template <int E>
__device__ __forceinline__ void bf_item_order(bool has_perm, int nlist, const uint32_t (&pw)[E],
                                              int (&ls)[E]) {
    const int i0 = E * (int)threadIdx.x;
#pragma unroll
    for (int j = 0; j < E; j++) ls[j] = i0 + j < nlist ? (has_perm ? (int)pw[j] : i0 + j) : -1;
}

// Count, then this: every work group loads all nlist counts, the item order
// and the lists' geometry next to its entries (one round trip, every load in
// flight at once), scans the counts in LDS (bf_offsets) and fills PER entries
// per thread and round from LDS alone.  Work group 0 writes the global offset
// arrays.
//
// Clearing the counts for the next call (a replayed graph relies on it, so
// the buffers cannot alternate): each group draws a ticket once its counts
// are in LDS; the group that draws the last one stores the zeros and resets
// the ticket.  No group waits for another, and within a group only the first
// wave, after its own fill, waits for the atomic to return.  The zeros need
// no inter-group release / acquire: a group's count loads have returned
// before its ticket is drawn (their values are in LDS before the barriers
// the draw follows), the zeros are stored only after the last draw has
// returned, and the last group reads nothing another group wrote in this
// launch — the zeros and the ticket are read by the next launch only, across
// a kernel boundary like every other store here.
template <int E, int PER>
__global__ __launch_bounds__(1024) void k_bucket_fill_scan(BFArgs a, uint32_t* counts,
                                                           const uint32_t* __restrict__ pos,
                                                           uint32_t* ticket) {
    extern __shared__ uint32_t bf_lds[];  // cnt[nlist], off[nlist], geo[nlist] {len, offset}
    __shared__ uint32_t wb[16], wi[16], s_last;
    uint32_t* cnt = bf_lds;
    uint32_t* off = bf_lds + a.nlist;
    uint2* geo = (uint2*)(bf_lds + 2 * a.nlist);
    const int t = threadIdx.x, l0 = E * t;
    const int qs = (a.QT & (a.QT - 1)) == 0 ? __builtin_ctz((unsigned)a.QT) : -1;
    uint32_t c[E], pw[E], gl[E], go[E];
    int ls[E], el[PER];
    uint32_t ep[PER];
    bf_load_words<E>(counts, a.nlist, c);
    bf_load_words<E>(a.perm ? a.perm : counts, a.nlist, pw);
    bf_load_words<E>(a.list_len, a.nlist, gl);
    bf_load_words<E>(a.list_off, a.nlist, go);
    // (the slot of an entry that was not counted is stale; bf_store ignores it)
    auto load = [&](int64_t base) {
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int64_t e = min(base + (int64_t)j * 1024 + t, a.total - 1);
            el[j] = a.assign[e];
            ep[j] = pos[e];
        }
        // both words are looked at here, so they are waited for here, ahead of
        // the stores: a wait placed among the stores would wait for those too
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const bool in = el[j] >= 0 && el[j] < a.nlist;
            el[j] = in ? el[j] : -1;
            ep[j] = in ? ep[j] : 0u;
        }
    };
    int64_t base = (int64_t)blockIdx.x * 1024 * PER;
    load(base);
#pragma unroll
    for (int j = 0; j < E; j++) {
        if (l0 + j < a.nlist) {
            cnt[l0 + j] = c[j];
            geo[l0 + j] = make_uint2(gl[j], go[j]);
        } else {
            c[j] = 0u;
        }
    }
    bf_item_order<E>(a.perm != nullptr, a.nlist, pw, ls);
    __syncthreads();
    // The draw: issued here, looked at after the fill, so that nothing waits
    // for the atomic's round trip.  tk is thread 0's alone (no value on the
    // other path, so no copy that would wait for it where the branch ends),
    // and the zero from a register the compiler cannot see through keeps the
    // address from counting as uniform: for a uniform address the compiler
    // folds the wave's lanes into one atomic and reads its result back at once.
    uint32_t tk, zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
    if (t == 0)
        tk = __hip_atomic_fetch_add(ticket + zero, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bf_offsets<E>(a, cnt, off, wb, wi, c, ls, qs, blockIdx.x == 0);
    for (;;) {
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int64_t e = base + (int64_t)j * 1024 + t;
            if (e < a.total) bf_store(a, cnt, off, geo, qs, e, el[j], ep[j]);
        }
        base += (int64_t)gridDim.x * 1024 * PER;
        if (base >= a.total) break;
        load(base);
    }
    if (t == 0) s_last = tk == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (s_last) {  // clear where the draw was the last
        const int n4 = a.nlist & ~3;
        for (int i = 4 * t; i < n4; i += 4096) *(uint4*)(counts + i) = make_uint4(0u, 0u, 0u, 0u);
        if (t < 4 && n4 + t < a.nlist) counts[n4 + t] = 0u;
        if (t == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One work group for the whole stage (at most 1024 PER entries): the LDS
// histogram of k_bucket_count_lds with the slots kept in registers, the scan,
// the fill.  The global counts and the slot array are not touched.  The
// lists' geometry goes through LDS here too (loaded beside the entries), so
// the histogram follows one round trip to memory instead of a gather of the
// list lengths after the assignment's.
template <int E, int PER>
__global__ __launch_bounds__(1024) void k_bucket_one(BFArgs a) {
    extern __shared__ uint32_t bf_lds[];  // cnt[nlist], off[nlist], geo[nlist] {len, offset}
    __shared__ uint32_t wb[16], wi[16];
    uint32_t* cnt = bf_lds;
    uint32_t* off = bf_lds + a.nlist;
    uint2* geo = (uint2*)(bf_lds + 2 * a.nlist);
    const int t = threadIdx.x, l0 = E * t;
    const int qs = (a.QT & (a.QT - 1)) == 0 ? __builtin_ctz((unsigned)a.QT) : -1;
    uint32_t pw[E], gl[E], go[E], ep[PER];
    int ls[E], el[PER];
#pragma unroll
    for (int j = 0; j < PER; j++)
        el[j] = a.assign[min((int64_t)j * 1024 + t, a.total - 1)];
    bf_load_words<E>(a.perm ? a.perm : a.list_len, a.nlist, pw);
    bf_load_words<E>(a.list_len, a.nlist, gl);
    bf_load_words<E>(a.list_off, a.nlist, go);
#pragma unroll
    for (int j = 0; j < E; j++) {
        if (l0 + j < a.nlist) {
            cnt[l0 + j] = 0u;
            geo[l0 + j] = make_uint2(gl[j], go[j]);
        }
    }
    bf_item_order<E>(a.perm != nullptr, a.nlist, pw, ls);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int l = el[j];
        // an empty list is no list, nor is what lies past the batch
        const bool ok = (int64_t)j * 1024 + t < a.total && l >= 0 && l < a.nlist && geo[l].x > 0u;
        el[j] = ok ? l : -1;
        ep[j] = ok ? atomicAdd(&cnt[l], 1u) : 0u;
    }
    __syncthreads();
    uint32_t c[E];
#pragma unroll
    for (int j = 0; j < E; j++) c[j] = l0 + j < a.nlist ? cnt[l0 + j] : 0u;
    bf_offsets<E>(a, cnt, off, wb, wi, c, ls, qs, true);
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int64_t e = (int64_t)j * 1024 + t;
        if (e < a.total) bf_store(a, cnt, off, geo, qs, e, el[j], ep[j]);
    }
}

__global__ void k_stamp(unsigned long long* out) { *out = __builtin_amdgcn_s_memrealtime(); }
void device_stamp(unsigned long long* out, hipStream_t s) {
    k_stamp<<<dim3(1), dim3(1), 0, s>>>(out);
    HIP_LAUNCH_CHECK();
}

// grid-stride partial counts per thread, one atomic pair per work-group
__global__ __launch_bounds__(256) void k_ivf_visit_stats(const int32_t* __restrict__ assign,
                                                         int64_t total,
                                                         const uint32_t* __restrict__ list_len,
                                                         int nlist,
                                                         const uint32_t* __restrict__ lim,
                                                         unsigned long long* __restrict__ stats) {
    unsigned long long nv = 0, nd = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int l = assign[e];
        uint32_t len = 0;
        if (l >= 0 && l < nlist) len = lim ? lim[e] : list_len[l];
        nv += len > 0 ? 1 : 0;
        nd += len;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        nv += __shfl_xor(nv, m);
        nd += __shfl_xor(nd, m);
    }
    __shared__ unsigned long long red[2][4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][w] = nv;
        red[1][w] = nd;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        const unsigned long long b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (a) {
            atomicAdd(&stats[0], a);
            atomicAdd(&stats[1], b);
        }
    }
}

void ivf_visit_stats(const int32_t* assign, int64_t total, const uint32_t* list_len, int nlist,
                     const uint32_t* lim, unsigned long long* stats, hipStream_t s) {
    if (total <= 0) return;
    const int64_t grid = std::min<int64_t>(cdiv(total, 256), 1024);
    k_ivf_visit_stats<<<kgrid(grid, 256), dim3(256), 0, s>>>(assign, total, list_len, nlist,
                                                                 lim, stats);
    HIP_LAUNCH_CHECK();
}

// one thread per query: faiss/IndexIVF.cpp:609-622 (nscan, list_size_max)
__global__ void k_probe_limits(const int32_t* __restrict__ assign, int64_t n, int nprobe,
                               const uint32_t* __restrict__ list_len, int nlist,
                               int64_t max_codes, int32_t* __restrict__ assign_out,
                               uint32_t* __restrict__ lim) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    int64_t nscan = 0;
    for (int r = 0; r < nprobe; r++) {
        const int64_t e = q * nprobe + r;
        const int l = assign[e];
        const bool ok = l >= 0 && l < nlist && nscan < max_codes;
        const uint32_t len = ok ? list_len[l] : 0u;
        const uint32_t take = (uint32_t)min((int64_t)len, max_codes - nscan);
        assign_out[e] = ok ? l : -1;
        lim[e] = take;
        nscan += take;
    }
}

void probe_limits(const int32_t* assign, int64_t n, int nprobe, const uint32_t* list_len,
                  int nlist, int64_t max_codes, int32_t* assign_out, uint32_t* lim,
                  hipStream_t s) {
    if (n <= 0) return;
    k_probe_limits<<<kgrid(cdiv(n, 256), 256), dim3(256), 0, s>>>(
            assign, n, nprobe, list_len, nlist, max_codes, assign_out, lim);
    HIP_LAUNCH_CHECK();
}

namespace {
// the LDS of the scan inside the fill, four words per list (count, offset,
// length, arena offset): past 64 KB with the static words (4096 lists; 128 KB
// at 8192) the dynamic limit is raised, as for k_bucket_count_lds
template <class K>
size_t bf_lds_bytes(K kernel, int nlist) {
    const size_t lds = sizeof(uint32_t) * 4 * (size_t)nlist;
    if (lds + 1024 > 65536)
        HIP_CHECK(hipFuncSetAttribute((const void*)kernel,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return lds;
}
template <int E, int PER>
void bucket_fill_scan(const BFArgs& a, const IVFBuckets& b, hipStream_t s) {
    // at most 512 work groups, each looping over its rounds of entries
    const int64_t groups = std::min<int64_t>(cdiv(a.total, 1024 * PER), 512);
    const size_t lds = bf_lds_bytes(k_bucket_fill_scan<E, PER>, a.nlist);
    k_bucket_fill_scan<E, PER><<<dim3((unsigned)groups), dim3(1024), lds, s>>>(a, b.counts, b.cursor,
                                                                             b.ticket);
}
template <int E, int PER>
void bucket_one(const BFArgs& a, hipStream_t s) {
    const size_t lds = bf_lds_bytes(k_bucket_one<E, PER>, a.nlist);
    k_bucket_one<E, PER><<<dim3(1), dim3(1024), lds, s>>>(a);
}
}  // namespace

void ivf_bucket(const int32_t* assign, int64_t n, int nprobe, const uint32_t* list_len,
                const uint32_t* list_off, int nlist, int QT, IVFBuckets b, hipStream_t s) {
    int64_t total = n * nprobe;
    FAISS_THROW_IF_NOT_MSG(total < (1ll << 32), "n * nprobe must fit in 32 bits");
    // up to BF_MAXL lists the fill scans the counts itself (no scan launch)
    const bool fused = total > 0 && nlist <= BF_MAXL && !b.item_list;
    const BFArgs fa{assign,     total,      list_len,  list_off,  nlist,          QT,
                    b.bucket_off, b.item_off, b.item_ctr, b.perm,    b.entries,      b.item_entries,
                    b.item_desc, b.mark_keys, b.mark_recs, b.mark_ke};
    if (fused && total <= BF_ONE_MAX) {
        // one work group, one launch; the counts stay zero and unread
        const int64_t per = (int64_t)cdiv(total, 1024);
        if (nlist <= 4096) {
            if (per <= 4) bucket_one<4, 4>(fa, s);
            else if (per <= 8) bucket_one<4, 8>(fa, s);
            else bucket_one<4, 16>(fa, s);
        } else {
            if (per <= 4) bucket_one<8, 4>(fa, s);
            else if (per <= 8) bucket_one<8, 8>(fa, s);
            else bucket_one<8, 16>(fa, s);
        }
        HIP_LAUNCH_CHECK();
        return;
    }
    if (!b.counts_next) HIP_CHECK(hipMemsetAsync(b.counts, 0, sizeof(uint32_t) * nlist, s));
    if (total > 0) {
        // entries per thread: enough work groups to spread the histogram
        // merge's global atomics over the chip (FAISS_AMD_BC_PER: tuning)
        // (c2, 4096 lists: 4 -> 7.6 us, 16 -> 12.9 us; c5, 65536 lists in 4
        // LDS ranges that each read every entry: 16 -> 162 us, 4 -> 233 us,
        // one global atomic per entry 254 us)
        const char* pe = getenv("FAISS_AMD_BC_PER");
        const int per = pe ? atoi(pe) : nlist > BC_MAXL ? 16 : 4;
        {
        // beyond 16384 lists: 32768-list ranges in 128 KB of LDS (half the
        // passes over the entries; FAISS_AMD_BC_BIG=0: 64 KB ranges)
        const char* be = getenv("FAISS_AMD_BC_BIG");
        const int maxl = nlist > BC_MAXL && !(be && !strcmp(be, "0")) ? BC_MAXL_BIG : BC_MAXL;
        const int nr2 = (int)cdiv(nlist, maxl);
        const size_t lds = sizeof(uint32_t) * std::min(nlist, maxl);
#define BCL(P)                                                                              \
    do {                                                                                    \
        if (lds > 65536)                                                                    \
            HIP_CHECK(hipFuncSetAttribute((const void*)k_bucket_count_lds<P>,               \
                                          hipFuncAttributeMaxDynamicSharedMemorySize,       \
                                          (int)lds));                                       \
        k_bucket_count_lds<P><<<dim3((unsigned)cdiv(total, 1024 * P), (unsigned)nr2),       \
                                dim3(1024), lds, s>>>(assign, total, list_len, nlist,       \
                                                      b.counts, b.cursor, maxl);            \
    } while (0)
        if (per >= 16) BCL(16);
        else if (per >= 8) BCL(8);
        else if (per >= 4) BCL(4);
        else if (per >= 2) BCL(2);
        else BCL(1);
#undef BCL
        HIP_LAUNCH_CHECK();
        }
    }
    // the fill scans the counts and the group with the last ticket clears
    // them (the self-cleaning counts of every caller; else the old kernels).
    // Two entries per thread while that gives every CU at most one work
    // group, else four.
    if (fused && b.ticket && b.counts_next == b.counts) {
        const bool two = cdiv(total, 2048) <= 256;
        if (nlist <= 4096) {
            if (two) bucket_fill_scan<4, 2>(fa, b, s);
            else bucket_fill_scan<4, 4>(fa, b, s);
        } else {
            if (two) bucket_fill_scan<8, 2>(fa, b, s);
            else bucket_fill_scan<8, 4>(fa, b, s);
        }
        HIP_LAUNCH_CHECK();
        return;
    }
    // beyond 8192 lists (and up to 64 groups of 4096): the scan over many
    // work groups, its block totals after the work counter (b.scan_tmp);
    // FAISS_AMD_SCAN_PAR=0: the single-group scan
    const char* pp = getenv("FAISS_AMD_SCAN_PAR");
    const int nbs = (int)cdiv(nlist, 4096);
    if (nlist > 8192 && nbs <= 64 && b.scan_tmp && !b.item_list && !(pp && !strcmp(pp, "0"))) {
        k_bucket_scan_part<4><<<dim3((unsigned)nbs), dim3(1024), 0, s>>>(
                b.counts, nlist, QT, b.bucket_off, b.item_off, b.perm, b.scan_tmp);
        HIP_LAUNCH_CHECK();
        k_bucket_scan_fix<4><<<dim3((unsigned)nbs), dim3(1024), 0, s>>>(
                nlist, b.bucket_off, b.item_off, b.perm, b.scan_tmp, b.counts_next, b.item_ctr);
        HIP_LAUNCH_CHECK();
    } else {
#define BSCAN(E)                                                                            \
    k_bucket_scan<E><<<dim3(1), dim3(1024), 0, s>>>(b.counts, nlist, QT, b.bucket_off,         \
                                                    b.item_off, b.item_list, b.counts_next,    \
                                                    b.item_ctr, b.perm)
    // counts per thread: 4 up to 4096 lists, else 16 (FAISS_AMD_SCAN_E: tuning)
    const char* se = getenv("FAISS_AMD_SCAN_E");
    const int E = se ? atoi(se) : nlist <= 4096 ? 4 : 16;
    if (E >= 16) BSCAN(16);
    else if (E >= 8) BSCAN(8);
    else BSCAN(4);
#undef BSCAN
    HIP_LAUNCH_CHECK();
    }
    if (total > 0) {
        k_bucket_fill<<<kgrid(cdiv(total, 256), 256), dim3(256), 0, s>>>(
                assign, total, list_len, nlist, QT, b.bucket_off, b.item_off, b.cursor, b.entries,
                b.item_entries, b.item_desc, b.counts, list_off, b.mark_keys, b.mark_recs,
                b.mark_ke);
        HIP_LAUNCH_CHECK();
    }
}


}  // namespace kern
}  // namespace faiss_amd
