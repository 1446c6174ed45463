// kernels_pq_lut.hip — IVF-PQ list scan for packed codes (4 <= nbits < 8) with
// the (query, probe) tables in LDS, for gfx950.
//
// At 4..7 bits a table is M * 2^nbits floats (2 KB at PQ32x4): cheap to build,
// small enough to keep several in the LDS, and its sequential sum IS the
// reference's distance (pq_ref.h pq_code_sum_seq), so no filter, margin or
// certification is needed.  Three kernels, every key exact:
//
//  1. k_lut_bound, one wave per query: the general path's scan
//     (pq_tables.h) over the query's first `nb` probes gives tau[q], the k-th
//     smallest exact key among them — an upper bound of the final k-th key
//     (fewer than k admissible rows there: further probes, then "no bound").
//  2. k_lut_scan, one 256-thread group per work item (list, <= QT queries
//     probing it; ivf_bucket's items, max_codes prefixes and IDSelector mask).
//     The list's part of table 1 (P, pq_tables.h) is built once per item; the
//     queries go LUT_QI = 4 at a time: their tables are built in the LDS
//     interleaved by query, lut4[m][j] = {t_q0, t_q1, t_q2, t_q3}, so a row's
//     decoded index fetches four queries' entries with one ds_read_b128, and
//     each thread takes one arena row: its code words as dwords, then the
//     M-step chain for the four queries (independent chains).  A key <= tau[q]
//     is appended to the query's candidate buffer with its arrival rank
//     (probe rank, arena row).
//  3. k_lut_select, one wave per query: exact_topk_resolve (exact_select.h)
//     over the buffer, which holds EVERY candidate with key <= tau >= the k-th
//     key, so the arrival-order tie rule is decided on complete information.
//     A query whose buffer overflowed (more than `cap` keys <= tau: planted
//     ties, or fewer than k admissible rows) is resolved by the same wave over
//     the general path's scan of all its probes.
//
// The answer equals the general exact scan's (kernels_exact.hip) bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "common.h"
#include "exact_select.h"
#include "kernels.h"
#include "pq_ref.h"
#include "pq_tables.h"
#include "ref_arith.h"
#include "wave_select.h"

namespace faiss_amd {
namespace kern {

namespace {

constexpr int LUT_QI = 4;     // queries per table pass (one ds_read_b128 per lookup)
constexpr int LUT_MAXW = 16;  // code dwords per arena row (code stride <= 64 B)

struct LutArgs {
    ExactScanArgs a;
    uint32_t* tau;    // [n] bound keys
    uint32_t* cnt;    // [n] candidates offered per query (may exceed cap)
    uint32_t* ckey;   // [n][cap] exact keys (ex_key)
    uint32_t* crank;  // [n][cap] probe ranks
    uint32_t* crow;   // [n][cap] arena rows
    int cap;
    int nb;  // probes of the bound pass
};

// key of the wave queues (wave_select.h to_key) from an ex_key
template <bool L2>
__device__ __forceinline__ float lut_k1(uint32_t key) {
    return L2 ? ex_dis(key, true) : -ex_dis(key, false);
}

// One wave (a 64-thread group): the rows of probe p of query q through the
// general path's table and code sum; f(ok, key, arena row) per lane,
// wave-uniform iteration.  ok: inside the scanned prefix, inside the
// IDSelector, and admissible for the reference heap.
template <bool L2, class F>
__device__ __forceinline__ void lut_probe_rows(const ExactScanArgs& a, int64_t q, int p,
                                               float* lut, F&& f) {
    const int64_t e = q * a.np + p;
    const int32_t key = a.assign[e];
    if (key < 0 || key >= a.nlist) return;
    const uint32_t full = a.list_len[key];
    const uint32_t len = a.lim ? min(a.lim[e], full) : full;
    if (len == 0) return;
    const float d0 = ex_pq_tables<L2, 0, 64>(a.x + q * a.ldx, a.ldx, a.d, key,
                                             a.cdis ? a.cdis[e] : 0.f, a.pq, lut);
    const uint32_t off = a.list_off[key];
    const int lane = threadIdx.x;
    for (uint32_t r0 = 0; r0 < len; r0 += 64) {
        const uint32_t r = r0 + lane, row = off + r;
        uint32_t kk = EX_SKIP;
        if (r < len && (!a.sel || a.sel[row]))
            kk = ex_key(d0 + ex_pq_code<0>(lut, a.pq, a.pq.codes + (int64_t)row * a.pq.cs), L2);
        f(kk != EX_SKIP, kk, row);
    }
}

template <bool L2>
__global__ __launch_bounds__(64) void k_lut_bound(LutArgs g) {
    extern __shared__ float lut[];
    const ExactScanArgs& a = g.a;
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    float fd = WS_INF, td = WS_INF;
    long long fi = WS_NOID, ti = WS_NOID;
    int seen = 0;
    for (int p = 0; p < a.np && (p < g.nb || seen < a.k); p++)
        lut_probe_rows<L2>(a, q, p, lut, [&](bool ok, uint32_t kk, uint32_t row) {
            seen += __popcll(__ballot(ok));
            wave_offer(fd, fi, ok ? lut_k1<L2>(kk) : WS_INF,
                       ok ? (((long long)p << 32) | row) : WS_NOID, td, ti, a.k, lane);
        });
    const float v = __shfl(fd, a.k - 1);
    const long long vi = shfl_ll(fi, a.k - 1);
    if (lane == 0) {
        uint32_t t = EX_SKIP - 1u;  // fewer than k admissible rows: no bound
        if (vi != WS_NOID) t = L2 ? ex_key(v, true) : ex_key(-v, false);
        g.tau[q] = t;
    }
}

template <bool L2>
__global__ __launch_bounds__(256) void k_lut_scan(LutArgs g, const uint32_t* __restrict__ item_off,
                                                  const ItemDesc* __restrict__ item_desc,
                                                  const uint32_t* __restrict__ item_entries,
                                                  int QT) {
    extern __shared__ float4 lut4[];  // [M * ksub] | P [M * ksub] | xs [QI][ldx] | rs [QI][ldx]
    __shared__ float g_d0[LUT_QI];
    __shared__ uint32_t g_tau[LUT_QI], g_len[LUT_QI], g_e[LUT_QI];
    const ExactScanArgs& a = g.a;
    const ExactPQ& pq = a.pq;
    const int M = pq.M, dsub = pq.dsub, nbits = pq.nbits, ME = M << nbits;
    const int ldx = a.ldx, np = a.np;
    float* Pl = (float*)(lut4 + ME);
    float* xs = Pl + ME;
    float* rs = xs + LUT_QI * ldx;
    const int tid = threadIdx.x;
    const bool t1 = L2 && pq.by_residual && pq.table1;
    const int NW = pq.cs >> 2;
    const uint32_t mask = (1u << nbits) - 1u;
    const uint32_t nitems = item_off[a.nlist];
    for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
        const ItemDesc dsc = item_desc[it];
        const float* yc = pq.cent + (int64_t)dsc.l * pq.ldcent;
        __syncthreads();  // the previous item's rows are done with Pl
        if (t1)
            for (int ent = tid; ent < ME; ent += 256)
                Pl[ent] = pq_list_term(yc + (ent >> nbits) * dsub,
                                       pq.pq_cent + (int64_t)ent * dsub, dsub);
        for (uint32_t g0 = 0; g0 < dsc.nq; g0 += LUT_QI) {
            __syncthreads();  // the previous pass's rows are done with the tables
            for (int i = tid; i < LUT_QI * ldx; i += 256) {
                const int qi = i / ldx, j = i - qi * ldx;
                float v = 0.f, r = 0.f;
                if (g0 + qi < dsc.nq) {
                    const uint32_t e = item_entries[(size_t)it * QT + g0 + qi];
                    v = a.x[(int64_t)(e / np) * ldx + j];
                    r = j < a.d ? v - yc[j] : 0.f;  // Index::compute_residual
                }
                xs[i] = v;
                rs[i] = r;
            }
            if (tid < LUT_QI) {
                const bool valid = g0 + tid < dsc.nq;
                const uint32_t e = valid ? item_entries[(size_t)it * QT + g0 + tid] : 0u;
                g_e[tid] = e;
                g_len[tid] = !valid ? 0u : a.lim ? min(a.lim[e], dsc.len) : dsc.len;
                g_tau[tid] = valid ? g.tau[e / np] : 0u;
            }
            __syncthreads();
            if (tid < LUT_QI)
                g_d0[tid] = pq_table_dis0<L2>(pq, xs + tid * ldx, yc, a.d,
                                              a.cdis ? a.cdis[g_e[tid]] : 0.f);
            for (int ent = tid; ent < ME; ent += 256) {
                const int mo = (ent >> nbits) * dsub;
                const float* c = pq.pq_cent + (int64_t)ent * dsub;
                float v[LUT_QI];
#pragma unroll
                for (int qi = 0; qi < LUT_QI; qi++)
                    v[qi] = t1 ? pq_table1_entry(xs + qi * ldx + mo, c, dsub, Pl[ent])
                               : pq_table_entry<L2>(pq, xs + qi * ldx + mo, rs + qi * ldx + mo,
                                                    yc + mo, c, dsub);
                lut4[ent] = make_float4(v[0], v[1], v[2], v[3]);
            }
            __syncthreads();
            uint32_t rows = 0;
#pragma unroll
            for (int qi = 0; qi < LUT_QI; qi++) rows = max(rows, g_len[qi]);
            for (uint32_t r = tid; r < rows; r += 256) {
                const uint32_t row = dsc.off + r;
                const uint32_t* cw = (const uint32_t*)(pq.codes + (int64_t)row * pq.cs);
                uint32_t cwr[LUT_MAXW];
#pragma unroll
                for (int w = 0; w < LUT_MAXW; w++) cwr[w] = w < NW ? cw[w] : 0u;
                // PQDecoderGeneric's bit stream through a 64-bit window; the
                // chains r = 0; r += tab[m][idx_m] of the four queries
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                unsigned long long win = 0ull;
                int have = 0, m = 0;
#pragma unroll
                for (int w = 0; w < LUT_MAXW; w++) {
                    if (w < NW) {
                        win |= (unsigned long long)cwr[w] << have;
                        have += 32;
                        while (have >= nbits && m < M) {
                            const uint32_t idx = (uint32_t)win & mask;
                            win >>= nbits;
                            have -= nbits;
                            const float4 t = lut4[(m << nbits) + idx];
                            s0 += t.x;
                            s1 += t.y;
                            s2 += t.z;
                            s3 += t.w;
                            m++;
                        }
                    }
                }
                const bool selok = !a.sel || a.sel[row];
                const float sum[LUT_QI] = {s0, s1, s2, s3};
#pragma unroll
                for (int qi = 0; qi < LUT_QI; qi++) {
                    const uint32_t kk = ex_key(g_d0[qi] + sum[qi], L2);
                    if (selok && r < g_len[qi] && kk != EX_SKIP && kk <= g_tau[qi]) {
                        const uint32_t e = g_e[qi], q = e / np;
                        const uint32_t slot = atomicAdd(&g.cnt[q], 1u);
                        if (slot < (uint32_t)g.cap) {
                            const int64_t o = (int64_t)q * g.cap + slot;
                            g.ckey[o] = kk;
                            g.crank[o] = e - q * np;
                            g.crow[o] = row;
                        }
                    }
                }
            }
        }
    }
}

// exact_topk_resolve streams (exact_select.h): f(ok, k1, k2, arrival rank)
template <bool L2>
struct LutBufStream {
    const LutArgs& g;
    int64_t q;
    uint32_t cnt;
    int lane;
    template <class F>
    __device__ __forceinline__ void for_each(F f) {
        for (uint32_t c0 = 0; c0 < cnt; c0 += 64) {
            const uint32_t i = c0 + lane;
            const bool ok = i < cnt;
            const int64_t o = q * g.cap + (ok ? i : 0u);
            const uint32_t kk = g.ckey[o], row = g.crow[o];
            float k1;
            long long k2;
            to_key(L2, ex_dis(kk, L2), g.a.ids[row], k1, k2);
            f(ok, k1, k2, ((long long)g.crank[o] << 32) | row);
        }
    }
};

template <bool L2>
struct LutAllStream {
    const ExactScanArgs& a;
    int64_t q;
    float* lut;
    template <class F>
    __device__ __forceinline__ void for_each(F f) {
        for (int p = 0; p < a.np; p++)
            lut_probe_rows<L2>(a, q, p, lut, [&](bool ok, uint32_t kk, uint32_t row) {
                float k1 = WS_INF;
                long long k2 = WS_NOID;
                if (ok) to_key(L2, ex_dis(kk, L2), a.ids[row], k1, k2);
                f(ok, k1, k2, ((long long)p << 32) | row);
            });
    }
};

template <bool L2>
__global__ __launch_bounds__(64) void k_lut_select(LutArgs g, float* __restrict__ D,
                                                   int64_t* __restrict__ I) {
    extern __shared__ float lut[];
    const ExactScanArgs& a = g.a;
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t cnt = g.cnt[q];
    if (cnt <= (uint32_t)g.cap) {
        LutBufStream<L2> st{g, q, cnt, lane};
        exact_topk_resolve(st, a.k, L2, lane, true, D + q * a.k, I + q * a.k);
    } else {
        LutAllStream<L2> st{a, q, lut};
        exact_topk_resolve(st, a.k, L2, lane, true, D + q * a.k, I + q * a.k);
    }
    if (lane == 0 && a.qdone) a.qdone[q] = __builtin_amdgcn_s_memrealtime();
}

size_t lut_scan_lds(const ExactPQ& pq, int ldx) {
    return sizeof(float) * (5 * ((size_t)pq.M << pq.nbits) + 2 * (size_t)LUT_QI * ldx);
}

}  // namespace

bool ivfpq_lut_eligible(int M, int nbits, int code_stride, int ldx, int k) {
    if (nbits < 4 || nbits > 7 || k < 1 || k > IVFPQ_LUT_KMAX) return false;
    if (code_stride % 4 != 0 || code_stride > 4 * LUT_MAXW) return false;
    ExactPQ pq;
    pq.M = M;
    pq.nbits = nbits;
    return lut_scan_lds(pq, ldx) <= 60 * 1024;  // + the static arrays, under 64 KB
}

size_t ivfpq_lut_scratch_words(int64_t n) { return (size_t)n * (2 + 3 * (size_t)IVFPQ_LUT_CAP); }

void ivfpq_lut_search(const ExactScanArgs& a, const IVFBuckets& b, int64_t max_items, int QT,
                      uint32_t* scratch, float* D, int64_t* I, hipStream_t s) {
    if (a.n <= 0) return;
    FAISS_THROW_IF_NOT(ivfpq_lut_eligible(a.pq.M, a.pq.nbits, a.pq.cs, a.ldx, a.k));
    FAISS_THROW_IF_NOT(a.n * (int64_t)a.np < ((int64_t)1 << 32) && !a.store_pairs);
    LutArgs g;
    g.a = a;
    g.cap = IVFPQ_LUT_CAP;
    g.tau = scratch;
    g.cnt = g.tau + a.n;
    g.ckey = g.cnt + a.n;
    g.crank = g.ckey + a.n * g.cap;
    g.crow = g.crank + a.n * g.cap;
    // probes of the bound pass: with rows spread evenly over the probes about
    // k * np / nb keys fall under the bound; aim at an eighth of the buffer, and
    // never bound from one probe alone (measured at IVF4096,PQ32x4, nprobe 32,
    // k 10: one probe leaves 156 candidates per query but up to 7228, two
    // leave 73 and at most 516)
    g.nb = (int)std::min<int64_t>(
            a.np, std::max<int64_t>(2, cdiv(8 * (int64_t)a.k * a.np, g.cap)));
    HIP_CHECK(hipMemsetAsync(g.cnt, 0, sizeof(uint32_t) * a.n, s));
    const size_t lds1 = sizeof(float) * ex_pq_table_floats(a.pq.M, a.pq.nbits, a.ldx);
    const size_t lds2 = lut_scan_lds(a.pq, a.ldx);
    const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>(max_items, 1), 2048);
    if (a.l2) {
        k_lut_bound<true><<<kgrid(a.n, 64), dim3(64), lds1, s>>>(g);
        k_lut_scan<true><<<dim3(grid), dim3(256), lds2, s>>>(g, b.item_off, b.item_desc,
                                                             b.item_entries, QT);
        k_lut_select<true><<<kgrid(a.n, 64), dim3(64), lds1, s>>>(g, D, I);
    } else {
        k_lut_bound<false><<<kgrid(a.n, 64), dim3(64), lds1, s>>>(g);
        k_lut_scan<false><<<dim3(grid), dim3(256), lds2, s>>>(g, b.item_off, b.item_desc,
                                                              b.item_entries, QT);
        k_lut_select<false><<<kgrid(a.n, 64), dim3(64), lds1, s>>>(g, D, I);
    }
    HIP_LAUNCH_CHECK();
}

}  // namespace kern
}  // namespace faiss_amd
