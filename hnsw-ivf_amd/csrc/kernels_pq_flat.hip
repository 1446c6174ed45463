// kernels_pq_flat.hip — exact k-NN over a flat array of packed PQ codes
// (IndexPQ, 4 <= nbits <= 8, L2 and inner product) with the queries' distance
// tables resident in the 160 KiB LDS of gfx950.
//
// Arithmetic (faiss/impl/ProductQuantizer.cpp:555-738): the table entries in
// the fvec_L2sqr_ny / fvec_inner_products_ny order (pq_ref.h ny_entry; for
// dsub == 2 below 8 bits the sum of the two rounded terms, as the reference's
// AVX2 compute_PQ_dis_tables_dsub2), the
// code sum as pq_estimators_from_tables* states it: dis = 0; dis += t[m] in
// order, except byte codes with M % 4 == 0 and M > 4, where each group of four
// is summed first (dism = t0; dism += t1 .. t3; dis += dism).
//
// Work split.  Grid = (query group of QI queries) x (slab of code rows); a
// work group is four waves, wave w owns the w-th quarter of the slab as one
// contiguous run of rows, a lane one row per pass.  Slab rule: nslab =
// ceil(512 / groups) (two work groups per CU when the batch is one group),
// but no slab shorter than 1024 rows and none at all beyond ceil(ntotal /
// 1024); the slab length is rounded up to 256 rows.  A large batch therefore
// runs one slab per group and writes four partial results per query.
//
// Tables.  Each work group builds its QI queries' tables once, interleaved by
// query: tab[(m << nbits) + idx] holds QI floats, so one ds_read_b128 (QI = 4;
// two at QI = 8, a b64 / b32 at QI = 2 / 1) serves a lookup for every query of
// the group.  QI is the largest of 8, 4, 2, 1 (not above the batch rounded up
// to a power of two) whose tables + query staging + candidate buffers fit the
// dynamic LDS limit (raised with hipFuncSetAttribute): PQ32x8 holds 4 queries
// in 128 KiB, PQ64x8 2, PQ128x8 1, PQ32x4 8 in 16 KiB.  When a single table
// does not fit (PQ256x8) the same kernel runs with GT = true: QI = 4 and the
// work group's tables in global scratch (L2-resident), the LDS keeping staging
// and candidates.
//
// Codes.  A row's code is read as dwords in chunks of four (one 16-byte load
// where the stride is a multiple of 16); the chunks of a pass and the first
// chunk of the next pass form one stream, and chunk c + 1 is loaded before the
// chains of chunk c run.  Any code stride works (PQ96x8: six chunks).
//
// Selection (k <= PQ_FLAT_KSEL).  Rows arrive in id order and the reference
// admits a key only when strictly better than the heap top.  Per (wave,
// query) the LDS holds up to 128 candidates (key, row) in row order and a
// bound th: a key <= th is appended through a ballot prefix, so the order is
// the row order.  When fewer than 64 slots are left, the wave finds v, the
// k-th smallest key of the buffer, keeps every candidate with key < v and the
// first k (by row) with key == v, and sets th = v: at most 2k - 1 survive.
// Completeness of ties: a dropped candidate has k tied candidates with lower
// rows before it in its own run, so it is not among the first k arrivals with
// key <= v of the whole array either; that set and the keys below v are all
// the reference's heap result depends on (exact_select.h).  The partials of a
// query, in (slab, wave) order = row order, go through the general exact
// select (kernels_exact.hip refine_select: arrival rank = position), which
// resolves ties that straddle waves, slabs and the k boundary by that rule.
// k > PQ_FLAT_KSEL: the kernel writes the distances of a chunk of queries to
// global scratch and select_rows_exact picks from the dense rows.
//
// No host round trip: table build and scan are one kernel, the select the
// next launch; scratch is grow-only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "common.h"
#include "kernels.h"
#include "pq_ref.h"
#include "ref_arith.h"
#include "wave_select.h"

namespace faiss_amd {
namespace kern {

namespace {

constexpr int PF_C = 128;                        // candidate slots per (wave, query)
constexpr size_t PF_LDS_MAX = 159 * 1024;        // dynamic LDS of one work group
constexpr size_t PF_GT_BYTES = (size_t)256 << 20;     // global tables of one launch
constexpr size_t PF_DENSE_BYTES = (size_t)512 << 20;  // dense distances of one launch

struct PFArgs {
    PQFlatArgs a;
    int64_t slab_rows;  // multiple of 256
    int nslab;
    float* gtab;        // GT: QI * M * ksub floats per work group
    uint32_t* pkeys;    // [n][nslab * 4][PC]
    int64_t* plabels;
    int PC;
    float* dense;  // != nullptr: distances [n][ntotal] instead of partials
};

template <int QI>
__device__ __forceinline__ void pf_get(const float* tab, int ent, float (&t)[QI]) {
    if constexpr (QI == 1) {
        t[0] = tab[ent];
    } else if constexpr (QI == 2) {
        const float2 v = ((const float2*)tab)[ent];
        t[0] = v.x;
        t[1] = v.y;
    } else {
#pragma unroll
        for (int h = 0; h < QI / 4; h++) {
            const float4 v = ((const float4*)tab)[ent * (QI / 4) + h];
            t[4 * h] = v.x;
            t[4 * h + 1] = v.y;
            t[4 * h + 2] = v.z;
            t[4 * h + 3] = v.w;
        }
    }
}

template <int QI>
__device__ __forceinline__ void pf_add(const float* tab, int ent, float (&s)[QI]) {
    float t[QI];
    pf_get<QI>(tab, ent, t);
#pragma unroll
    for (int qi = 0; qi < QI; qi++) s[qi] += t[qi];
}

// One wave: buf[0 .. cnt) (row order, k <= cnt <= PF_C) -> the candidates
// below the k-th smallest key v and the first k at v, in row order; th = v.
__device__ __forceinline__ void pf_compact(uint2* buf, int& cnt, uint32_t& th, int k, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int p0 = lane, p1 = lane + 64;
    const uint2 e0 = p0 < cnt ? buf[p0] : make_uint2(EX_SKIP, 0u);
    const uint2 e1 = p1 < cnt ? buf[p1] : make_uint2(EX_SKIP, 0u);
    int lt0 = 0, le0 = 0, eb0 = 0, lt1 = 0, le1 = 0, eb1 = 0;
    for (int j = 0; j < cnt; j++) {
        const uint32_t kj = buf[j].x;
        lt0 += kj < e0.x;
        le0 += kj <= e0.x;
        eb0 += kj == e0.x && j < p0;
        lt1 += kj < e1.x;
        le1 += kj <= e1.x;
        eb1 += kj == e1.x && j < p1;
    }
    const unsigned long long b0 = __ballot(p0 < cnt && lt0 < k && k <= le0);
    const unsigned long long b1 = __ballot(p1 < cnt && lt1 < k && k <= le1);
    const uint32_t v = b0 ? (uint32_t)__shfl((int)e0.x, __ffsll((long long)b0) - 1)
                          : (uint32_t)__shfl((int)e1.x, __ffsll((long long)b1) - 1);
    const bool keep0 = p0 < cnt && (e0.x < v || (e0.x == v && eb0 < k));
    const bool keep1 = p1 < cnt && (e1.x < v || (e1.x == v && eb1 < k));
    const unsigned long long m0 = __ballot(keep0), m1 = __ballot(keep1);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n0 = __popcll(m0);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (keep0) buf[__popcll(m0 & below)] = e0;
    if (keep1) buf[n0 + __popcll(m1 & below)] = e1;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    cnt = n0 + __popcll(m1);
    th = v;
}

// G4: byte codes, M % 4 == 0, M > 4 (a dword is one group of four)
template <int QI, bool GT, bool G4>
__global__ __launch_bounds__(256) void k_pq_flat(PFArgs g) {
    extern __shared__ float4 pf_smem[];
    const PQFlatArgs& a = g.a;
    const int M = a.M, dsub = a.dsub, nbits = G4 ? 8 : a.nbits, ME = M << nbits;
    const int ldx = a.ldx;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float* smem = (float*)pf_smem;
    float* tab = GT ? g.gtab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)ME * QI
                    : smem;
    float* xs = GT ? smem : smem + (size_t)ME * QI;
    uint2* cand = (uint2*)(xs + (size_t)QI * ldx) + (size_t)wid * QI * PF_C;
    const int64_t q0 = (int64_t)blockIdx.x * QI;

    // ---- the group's query rows, then its tables (pq_ref.h entry order)
    for (int i = tid; i < QI * ldx; i += 256) {
        const int qi = i / ldx, j = i - qi * ldx;
        xs[i] = q0 + qi < a.n ? a.x[(q0 + qi) * ldx + j] : 0.f;
    }
    __syncthreads();
    // dsub == 2 below 8 bits: the reference's compute_PQ_dis_tables_dsub2
    // (faiss/utils/distances_simd.cpp:3616-3728) adds the two rounded terms
    const bool dsub2 = dsub == 2 && nbits < 8;
    for (int ent = tid; ent < ME; ent += 256) {
        const int mo = (ent >> nbits) * dsub;
        const float* c = a.pq_cent + (int64_t)ent * dsub;
#pragma unroll
        for (int qi = 0; qi < QI; qi++) {
            const float* xm = xs + qi * ldx + mo;
            float t;
            if (dsub2)
                t = a.l2 ? ref_term<true>(xm[0], c[0]) + ref_term<true>(xm[1], c[1])
                         : ref_term<false>(xm[0], c[0]) + ref_term<false>(xm[1], c[1]);
            else
                t = a.l2 ? ny_entry<true>(xm, c, dsub) : ny_entry<false>(xm, c, dsub);
            tab[(size_t)ent * QI + qi] = t;
        }
    }
    __syncthreads();

    // ---- this wave's run of rows
    const int64_t wrows = g.slab_rows >> 2;
    const int64_t r0 = (int64_t)blockIdx.y * g.slab_rows + wid * wrows;
    const int64_t r1 = min(r0 + wrows, a.ntotal);
    const int NW = a.cs >> 2, NC = (NW + 3) >> 2;
    const bool vec = (a.cs & 15) == 0;
    const uint32_t mask = (1u << nbits) - 1u;
    auto load_chunk = [&](int64_t row, int c) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row < r1) {
            const uint32_t* p = (const uint32_t*)(a.codes + row * a.cs) + 4 * c;
            if (vec) {
                v = *(const uint4*)p;
            } else {
                const int w = 4 * c;
                v.x = p[0];  // w < NW: c < NC
                if (w + 1 < NW) v.y = p[1];
                if (w + 2 < NW) v.z = p[2];
                if (w + 3 < NW) v.w = p[3];
            }
        }
        return v;
    };
    uint32_t th[QI];
    int cnt[QI];
#pragma unroll
    for (int qi = 0; qi < QI; qi++) {
        th[qi] = EX_SKIP - 1u;
        cnt[qi] = 0;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    uint4 nxt = load_chunk(r0 + lane, 0);
    for (int64_t rb = r0; rb < r1; rb += 64) {
        const int64_t row = rb + lane;
        float s[QI];
#pragma unroll
        for (int qi = 0; qi < QI; qi++) s[qi] = 0.f;
        unsigned long long win = 0ull;
        int have = 0, m = 0;
        for (int c = 0; c < NC; c++) {
            const uint4 cur = nxt;
            nxt = c + 1 < NC ? load_chunk(row, c + 1) : load_chunk(row + 64, 0);
            const uint32_t cw[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (4 * c + j >= NW) continue;
                if constexpr (G4) {
                    float t[QI];
                    pf_get<QI>(tab, (m << 8) + (int)(cw[j] & 255u), t);
                    pf_add<QI>(tab, ((m + 1) << 8) + (int)((cw[j] >> 8) & 255u), t);
                    pf_add<QI>(tab, ((m + 2) << 8) + (int)((cw[j] >> 16) & 255u), t);
                    pf_add<QI>(tab, ((m + 3) << 8) + (int)(cw[j] >> 24), t);
#pragma unroll
                    for (int qi = 0; qi < QI; qi++) s[qi] += t[qi];
                    m += 4;
                } else {
                    // PQDecoderGeneric's bit stream through a 64-bit window
                    win |= (unsigned long long)cw[j] << have;
                    have += 32;
                    while (have >= nbits && m < M) {
                        const int idx = (int)((uint32_t)win & mask);
                        win >>= nbits;
                        have -= nbits;
                        pf_add<QI>(tab, (m << nbits) + idx, s);
                        m++;
                    }
                }
            }
        }
        if (g.dense) {
#pragma unroll
            for (int qi = 0; qi < QI; qi++)
                if (row < r1 && q0 + qi < a.n) g.dense[(q0 + qi) * a.ntotal + row] = s[qi];
            continue;
        }
#pragma unroll
        for (int qi = 0; qi < QI; qi++) {
            const uint32_t key = row < r1 ? ex_key(s[qi], a.l2 != 0) : EX_SKIP;
            const bool pass = key <= th[qi];
            const unsigned long long bm = __ballot(pass);
            if (bm) {
                uint2* buf = cand + qi * PF_C;
                if (pass) buf[cnt[qi] + __popcll(bm & below)] = make_uint2(key, (uint32_t)row);
                cnt[qi] += __popcll(bm);
                if (cnt[qi] > PF_C - 64) pf_compact(buf, cnt[qi], th[qi], a.k, lane);
            }
        }
    }
    if (g.dense) return;
    // ---- this run's partial of each query: at most 2k - 1 candidates
    const int64_t nparts = (int64_t)g.nslab * 4, part = (int64_t)blockIdx.y * 4 + wid;
#pragma unroll
    for (int qi = 0; qi < QI; qi++) {
        if (q0 + qi >= a.n) continue;
        uint2* buf = cand + qi * PF_C;
        if (cnt[qi] >= a.k) pf_compact(buf, cnt[qi], th[qi], a.k, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int64_t o = ((q0 + qi) * nparts + part) * g.PC;
        for (int i = lane; i < g.PC; i += 64) {
            const bool ok = i < cnt[qi];
            const uint2 e = ok ? buf[i] : make_uint2(EX_SKIP, 0u);
            g.pkeys[o + i] = e.x;
            g.plabels[o + i] = ok ? (int64_t)e.y : (int64_t)-1;
        }
    }
}

struct PFPlan {
    int QI = 1;
    bool gt = false, g4 = false, dense = false;
    size_t lds = 0;
};

size_t pf_lds(const PQFlatArgs& a, int QI, bool gt, bool dense) {
    const size_t ME = (size_t)a.M << a.nbits;
    return sizeof(float) * QI * ((gt ? 0 : ME) + (size_t)a.ldx) +
           (dense ? 0 : sizeof(uint2) * 4 * QI * PF_C);
}

PFPlan pf_plan(const PQFlatArgs& a) {
    PFPlan p;
    p.dense = a.k > PQ_FLAT_KSEL;
    p.g4 = a.nbits == 8 && a.M % 4 == 0 && a.M > 4;
    int qmax = 1;
    while (qmax < 8 && qmax < a.n) qmax *= 2;
    for (p.QI = qmax; p.QI >= 1; p.QI /= 2)
        if (pf_lds(a, p.QI, false, p.dense) <= PF_LDS_MAX) break;
    if (p.QI < 1) {
        p.gt = true;
        p.QI = 4;
    }
    p.lds = pf_lds(a, p.QI, p.gt, p.dense);
    FAISS_THROW_IF_NOT_FMT(p.lds <= PF_LDS_MAX,
                           "pq_flat_search: d = %d needs %zu bytes of LDS for its query rows",
                           a.d, p.lds);
    return p;
}

template <int QI, bool GT, bool G4>
void pf_launch(const PFArgs& g, int64_t groups, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024)
        HIP_CHECK(hipFuncSetAttribute((const void*)k_pq_flat<QI, GT, G4>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    FAISS_THROW_IF_NOT(groups >= 1 && groups < ((int64_t)1 << 31) && g.nslab >= 1 &&
                       g.nslab <= 65535);
    k_pq_flat<QI, GT, G4><<<dim3((unsigned)groups, (unsigned)g.nslab), dim3(256), lds, s>>>(g);
    HIP_LAUNCH_CHECK();
}

template <bool G4>
void pf_dispatch(const PFPlan& p, const PFArgs& g, int64_t groups, hipStream_t s) {
    if (p.gt) return pf_launch<4, true, G4>(g, groups, p.lds, s);
    switch (p.QI) {
        case 8:
            return pf_launch<8, false, G4>(g, groups, p.lds, s);
        case 4:
            return pf_launch<4, false, G4>(g, groups, p.lds, s);
        case 2:
            return pf_launch<2, false, G4>(g, groups, p.lds, s);
        default:
            return pf_launch<1, false, G4>(g, groups, p.lds, s);
    }
}

}  // namespace

int pq_flat_queries_per_group(const PQFlatArgs& a, bool* global_tables) {
    const PFPlan p = pf_plan(a);
    if (global_tables) *global_tables = p.gt;
    return p.QI;
}

void pq_flat_search(const PQFlatArgs& a, DeviceBuffer& s_part, DeviceBuffer& s_tab,
                    DeviceBuffer& s_dense, float* D, int64_t* I, hipStream_t s) {
    if (a.n <= 0) return;
    FAISS_THROW_IF_NOT_FMT(a.k >= 1 && a.k <= kMaxKExact, "k = %d must be in [1, %d]", a.k,
                           kMaxKExact);
    FAISS_THROW_IF_NOT(a.nbits >= 4 && a.nbits <= 8 && a.cs % 4 == 0 &&
                       a.cs * 8 >= a.M * a.nbits && a.ldx % 4 == 0 && a.ldx >= a.d);
    FAISS_THROW_IF_NOT_MSG(a.ntotal < ((int64_t)1 << 32), "pq_flat_search: ntotal must be < 2^32");
    const PFPlan p = pf_plan(a);
    const size_t tab_bytes = sizeof(float) * p.QI * ((size_t)a.M << a.nbits);
    // queries of one launch: the scratch sizes, and a 32-bit partial count
    int64_t qc = std::min<int64_t>(a.n, 65536);
    if (p.dense)
        qc = std::min<int64_t>(qc, std::max<int64_t>(1, PF_DENSE_BYTES / (4 * std::max<int64_t>(a.ntotal, 1))));
    if (p.gt) qc = std::min<int64_t>(qc, std::max<int64_t>(1, PF_GT_BYTES / tab_bytes) * p.QI);
    if (qc < a.n) qc = std::max<int64_t>(p.QI, qc / p.QI * p.QI);
    const int64_t groups_max = (int64_t)cdiv((size_t)qc, (size_t)p.QI);
    PFArgs g;
    g.nslab = (int)std::max<int64_t>(
            1, std::min<int64_t>((int64_t)cdiv(512, (size_t)groups_max), a.ntotal / 1024));
    if (p.gt)
        g.nslab = (int)std::max<int64_t>(
                1, std::min<int64_t>(g.nslab, (int64_t)(PF_GT_BYTES / tab_bytes) / groups_max));
    g.slab_rows = (int64_t)roundup(cdiv((size_t)std::max<int64_t>(a.ntotal, 1), (size_t)g.nslab), 256);
    g.nslab = (int)cdiv((size_t)std::max<int64_t>(a.ntotal, 1), (size_t)g.slab_rows);
    g.PC = 2 * a.k;
    const int64_t k_base = (int64_t)g.nslab * 4 * g.PC;
    if (p.dense) {
        s_dense.reserve(sizeof(float) * (size_t)qc * std::max<int64_t>(a.ntotal, 1));
    } else {
        s_part.reserve((sizeof(uint32_t) + sizeof(int64_t)) * (size_t)qc * k_base);
    }
    if (p.gt) s_tab.reserve(tab_bytes * groups_max * g.nslab);
    g.gtab = p.gt ? s_tab.as<float>() : nullptr;
    g.dense = p.dense ? s_dense.as<float>() : nullptr;
    g.plabels = s_part.as<int64_t>();
    g.pkeys = p.dense ? nullptr : (uint32_t*)(g.plabels + qc * k_base);
    for (int64_t q = 0; q < a.n; q += qc) {
        g.a = a;
        g.a.x = a.x + q * a.ldx;
        g.a.n = std::min(qc, a.n - q);
        const int64_t groups = (int64_t)cdiv((size_t)g.a.n, (size_t)p.QI);
        if (p.g4) pf_dispatch<true>(p, g, groups, s);
        else pf_dispatch<false>(p, g, groups, s);
        if (p.dense) {
            // (no rows: the select over zero columns pads every slot)
            select_rows_exact<int64_t>(g.dense, g.a.n, a.ntotal, a.ntotal, a.k, a.l2, 0,
                                       D + q * a.k, I + q * a.k, a.k, s);
        } else {
            refine_select(g.pkeys, g.plabels, g.a.n, k_base, a.k, a.l2, D + q * a.k, I + q * a.k,
                          s);
        }
    }
}

}  // namespace kern
}  // namespace faiss_amd
