// kernels_binary.hip — exact Hamming k-NN over packed bit vectors
// (IndexBinaryFlat, IndexBinaryIVF).
//
// Layout.  A vector of d bits is W = ceil(d / 32) dwords, zero padded (padding
// both operands leaves the distance unchanged).  The flat index is one array
// [ntotal][W]; the IVF lists are runs of one arena [rows][W], list l at rows
// [list_off[l], list_off[l] + list_len[l]) (int64 offsets).
//
// One scan kernel (k_bin_scan<QT, NWV, IVF>) serves both.  A work group has
// QT queries in LDS and a run of rows, cut into NWV contiguous pieces, one per
// wave.  A lane owns one row: 16 of its dwords sit in registers (dwordx4 loads
// when W % 4 == 0; consecutive lanes take consecutive rows), and the lane
// walks the QT queries, reading every query word at a wave-uniform LDS address
// (a broadcast) and issuing one xor and one accumulating popcount per word and
// pair.  Codes wider than 16 dwords loop over 16-dword chunks with a running
// count per query.
//   flat: grid = (tile of QT = 16 queries, slab of rows), four waves; QT = 8
//         when 16 query rows and their candidate buffers exceed the LDS
//         (d > 48640 bits);
//   IVF:  grid = (query, probe), QT = 1; the run is the probed list, one wave,
//         or four when the longest list has more than 1024 rows.
//
// Selection.  Distances are integers in [0, d]; as floats they are exact, so
// the key is the exact select's 32-bit key (wave_select.h ex_key) and every
// tie rule is a matter of arrival order and labels:
//   k <= BIN_KSEL: per (wave, query) the LDS holds up to 128 candidates (key,
//     row) in arrival order and a bound th; a key <= th is appended through a
//     ballot prefix.  With fewer than 64 free slots the wave keeps the
//     candidates below v, the k-th smallest key of the buffer, and the first k
//     at v, and sets th = v (at most 2k - 1 survive).  A dropped candidate has
//     k candidates with key <= v before it in its own run, so it is not among
//     the first k arrivals with key <= T of the whole scan either.  The
//     partials of a query, laid out in arrival order (slab, wave) or (probe,
//     wave), go through refine_select (kernels_exact.hip), which applies the
//     reference heap's rule: everything below the k-th key T, and of the ties
//     among the first k arrivals with key <= T those with the smallest labels.
//   k > BIN_KSEL: the flat scan writes dense float distances for
//     select_rows_exact; the IVF scan writes every (key, label) at
//     [probe][offset in list] of a per-query table for refine_select.  That
//     table has nprobe x (longest list) slots of 12 bytes whatever the probed
//     lists hold, so one long list with a large nprobe makes it large; a
//     table over 4 GiB for a single query is refused by name.
// Labels.  Flat: the row number (both use_heap modes: k smallest by (distance,
// id)).  IVF with use_heap: the stored id.  IVF without (the reference's
// counting scan: k smallest by (distance, arrival)): the arrival position
// (probe << 32 | offset), which ascends along the arrival order, so the same
// select returns the first arrivals; k_bin_finish then replaces positions by
// ids.  k_bin_finish also turns the float distances into int32 in place
// (padding: INT32_MAX, -1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>

#include "common.h"
#include "kernels.h"
#include "wave_select.h"

namespace faiss_amd {
namespace kern {

namespace {

constexpr int BN_C = 128;   // candidate slots per (wave, query)
constexpr int BN_CH = 16;   // dwords of a row held in registers
constexpr int BN_QT = 16;   // queries per flat work group (8 when 16 do not fit the LDS)
constexpr size_t BN_LDS_MAX = 159 * 1024;
constexpr size_t BN_SCRATCH = (size_t)512 << 20;  // partials / dense tables of one launch

struct BinArgs {
    const uint32_t* x = nullptr;  // [n][W]
    int64_t n = 0;
    int W = 0, k = 0;
    const uint32_t* codes = nullptr;  // [rows][W]
    // flat
    int64_t ntotal = 0, slab_rows = 0;  // slab_rows: multiple of 256
    // IVF
    const int32_t* assign = nullptr;  // [n][np], -1 = none
    int np = 0, by_pos = 0;
    const int64_t* list_off = nullptr;
    const uint32_t* list_len = nullptr;
    const int64_t* ids = nullptr;
    // k <= BIN_KSEL: partials [n][nparts][PC]
    uint32_t* pkeys = nullptr;
    int64_t* plabels = nullptr;
    int PC = 0, nparts = 0;
    // k > BIN_KSEL: flat distances [n][ntotal]; IVF (key, label) [n][cap] at
    // p * maxlen + offset
    float* dense = nullptr;
    uint32_t* ckeys = nullptr;
    int64_t* clabels = nullptr;
    int64_t cap = 0, maxlen = 0;
};

// One wave: buf[0 .. cnt) (arrival order, k <= cnt <= BN_C) -> the candidates
// below the k-th smallest key v and the first k at v, in arrival order; th = v.
__device__ __forceinline__ void bn_compact(uint2* buf, int& cnt, uint32_t& th, int k, int lane) {
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

__host__ __device__ inline size_t bn_xs_words(int QT, int W) {
    return ((size_t)QT * W + 1) & ~(size_t)1;  // the candidates after it are 8-byte aligned
}

template <int QT, int NWV, bool IVF>
__global__ __launch_bounds__(64 * NWV) void k_bin_scan(BinArgs g) {
    extern __shared__ uint32_t bn_smem[];
    const int W = g.W;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t* xs = bn_smem;  // [QT][W]
    uint2* cand = (uint2*)(xs + bn_xs_words(QT, W)) + (size_t)wid * QT * BN_C;
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    for (int i = tid; i < QT * W; i += 64 * NWV) {
        const int qi = i / W, j = i - qi * W;
        xs[i] = q0 + qi < g.n ? g.x[(q0 + qi) * W + j] : 0u;
    }
    __syncthreads();

    // ---- this work group's run of rows [base, base + len), this wave's piece
    int64_t base = 0, len = 0, wrows = 0;
    if constexpr (IVF) {
        const int32_t l = g.assign[q0 * g.np + blockIdx.y];
        if (l >= 0) {
            base = g.list_off[l];
            len = g.list_len[l];
        }
        wrows = (len + NWV - 1) / NWV;
    } else {
        base = (int64_t)blockIdx.y * g.slab_rows;
        len = min(g.slab_rows, g.ntotal - base);
        wrows = g.slab_rows / NWV;
    }
    const int64_t r0 = min((int64_t)wid * wrows, len), r1 = min(r0 + wrows, len);
    const bool vec = (W & 3) == 0;
    const bool partial = g.pkeys != nullptr;

    uint32_t th[QT];
    int cnt[QT];
#pragma unroll
    for (int qi = 0; qi < QT; qi++) {
        th[qi] = EX_SKIP - 1u;
        cnt[qi] = 0;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t rb = r0; rb < r1; rb += 64) {
        const int64_t r = rb + lane;  // relative to base
        const bool valid = r < r1;
        const uint32_t* p = g.codes + (base + (valid ? r : r0)) * W;
        uint32_t acc[QT];
#pragma unroll
        for (int qi = 0; qi < QT; qi++) acc[qi] = 0u;
        for (int c0 = 0; c0 < W; c0 += BN_CH) {
            uint32_t rw[BN_CH];
            const int nw = min(BN_CH, W - c0);  // wave-uniform
            if (vec) {
#pragma unroll
                for (int t = 0; t < BN_CH / 4; t++) {
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);
                    if (valid && 4 * t < nw) v = *(const uint4*)(p + c0 + 4 * t);
                    rw[4 * t] = v.x;
                    rw[4 * t + 1] = v.y;
                    rw[4 * t + 2] = v.z;
                    rw[4 * t + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < BN_CH; j++) rw[j] = valid && j < nw ? p[c0 + j] : 0u;
            }
            if (nw == BN_CH) {
#pragma unroll
                for (int qi = 0; qi < QT; qi++) {
                    const uint32_t* xq = xs + qi * W + c0;
                    uint32_t a = acc[qi];
#pragma unroll
                    for (int j = 0; j < BN_CH; j++) a += __popc(rw[j] ^ xq[j]);
                    acc[qi] = a;
                }
            } else {
#pragma unroll
                for (int qi = 0; qi < QT; qi++) {
                    const uint32_t* xq = xs + qi * W + c0;
                    uint32_t a = acc[qi];
#pragma unroll
                    for (int j = 0; j < BN_CH; j++)
                        if (j < nw) a += __popc(rw[j] ^ xq[j]);
                    acc[qi] = a;
                }
            }
        }
        if (!partial) {
#pragma unroll
            for (int qi = 0; qi < QT; qi++) {
                if (!valid || q0 + qi >= g.n) continue;
                if constexpr (IVF) {
                    const int64_t o = (q0 + qi) * g.cap + (int64_t)blockIdx.y * g.maxlen + r;
                    g.ckeys[o] = ex_key((float)acc[qi], true);
                    g.clabels[o] = g.by_pos ? (((int64_t)blockIdx.y << 32) | r) : g.ids[base + r];
                } else {
                    g.dense[(q0 + qi) * g.ntotal + base + r] = (float)acc[qi];
                }
            }
            continue;
        }
#pragma unroll
        for (int qi = 0; qi < QT; qi++) {
            const uint32_t key = valid ? ex_key((float)acc[qi], true) : EX_SKIP;
            const bool pass = key <= th[qi];
            const unsigned long long bm = __ballot(pass);
            if (bm) {
                uint2* buf = cand + qi * BN_C;
                if (pass) buf[cnt[qi] + __popcll(bm & below)] = make_uint2(key, (uint32_t)r);
                cnt[qi] += __popcll(bm);
                if (cnt[qi] > BN_C - 64) bn_compact(buf, cnt[qi], th[qi], g.k, lane);
            }
        }
    }
    if (!partial) return;
    // ---- this piece's partial of each query: at most 2k - 1 candidates
    const int64_t part = (int64_t)blockIdx.y * NWV + wid;
#pragma unroll
    for (int qi = 0; qi < QT; qi++) {
        if (q0 + qi >= g.n) continue;
        uint2* buf = cand + qi * BN_C;
        if (cnt[qi] >= g.k) bn_compact(buf, cnt[qi], th[qi], g.k, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int64_t o = ((q0 + qi) * g.nparts + part) * g.PC;
        for (int i = lane; i < g.PC; i += 64) {
            const bool ok = i < cnt[qi];
            const uint2 e = ok ? buf[i] : make_uint2(EX_SKIP, 0u);
            int64_t label = -1;
            if (ok) {
                if constexpr (IVF)
                    label = g.by_pos ? (((int64_t)blockIdx.y << 32) | e.y) : g.ids[base + e.y];
                else
                    label = base + e.y;
            }
            g.pkeys[o + i] = e.x;
            g.plabels[o + i] = label;
        }
    }
}

__global__ void k_bin_fill(uint32_t* keys, int64_t* labels, int64_t n) {
    GRID_STRIDE(i, n) {
        keys[i] = EX_SKIP;
        labels[i] = -1;
    }
}

// the select's float distances -> int32 in place; arrival positions -> ids
__global__ void k_bin_finish(int32_t* D, int64_t* I, int64_t n, int k, int by_pos,
                             const int32_t* assign, int np, const int64_t* list_off,
                             const int64_t* ids) {
    GRID_STRIDE(i, n * k) {
        const int64_t lab = I[i];
        const float dis = __int_as_float(D[i]);
        if (lab < 0) {
            D[i] = INT_MAX;
            I[i] = -1;
            continue;
        }
        D[i] = (int32_t)dis;
        if (by_pos) {
            const int64_t q = i / k;
            const int32_t l = assign[q * np + (lab >> 32)];
            I[i] = ids[list_off[l] + (lab & 0xffffffffll)];
        }
    }
}

// labels of the coarse search -> the probes scanned: lists in coarse order, and
// after the first list that brings the scanned rows to max_codes none
// (faiss/IndexBinaryIVF.cpp: whole lists are scanned, `nscan >= max_codes` ends
// the probe loop)
__global__ void k_bin_probes(const int64_t* coarse, int64_t n, int np, const uint32_t* list_len,
                             int nlist, int64_t max_codes, int32_t* assign) {
    GRID_STRIDE(q, n) {
        int64_t nscan = 0;
        bool stop = false;
        for (int p = 0; p < np; p++) {
            const int64_t l = coarse[q * np + p];
            const bool ok = !stop && l >= 0 && l < nlist;
            assign[q * np + p] = ok ? (int32_t)l : -1;
            if (ok) {
                nscan += list_len[l];
                if (max_codes && nscan >= max_codes) stop = true;
            }
        }
    }
}

// dynamic LDS of a work group: its queries, and for k <= BIN_KSEL the
// candidate buffers of its waves
size_t bn_lds(int QT, int NWV, int W, bool partial) {
    return sizeof(uint32_t) * bn_xs_words(QT, W) + (partial ? sizeof(uint2) * NWV * QT * BN_C : 0);
}

template <int QT, int NWV, bool IVF>
void bn_launch(const BinArgs& g, int64_t gx, int64_t gy, hipStream_t s) {
    const size_t lds = bn_lds(QT, NWV, g.W, g.pkeys != nullptr);
    FAISS_THROW_IF_NOT_FMT(lds <= BN_LDS_MAX, "binary scan: %zu bytes of LDS", lds);
    if (lds > 64 * 1024)
        HIP_CHECK(hipFuncSetAttribute((const void*)k_bin_scan<QT, NWV, IVF>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    FAISS_THROW_IF_NOT(gx >= 1 && gx < ((int64_t)1 << 31) && gy >= 1 && gy <= 65535);
    k_bin_scan<QT, NWV, IVF><<<dim3((unsigned)gx, (unsigned)gy), dim3(64 * NWV), lds, s>>>(g);
    HIP_LAUNCH_CHECK();
}

void bn_check(int64_t n, int d, int k) {
    FAISS_THROW_IF_NOT_FMT(k >= 1 && k <= kMaxKExact, "k = %d must be in [1, %d]", k, kMaxKExact);
    const bool d_ok = d >= 8 && d <= BIN_MAX_D && (d & 7) == 0;
    FAISS_THROW_IF_NOT_FMT(d_ok, "d = %d bits must be a multiple of 8 in [8, %d]", d, BIN_MAX_D);
}

}  // namespace

void binary_flat_search(const uint32_t* x, int64_t n, int d, const uint32_t* codes,
                        int64_t ntotal, int k, DeviceBuffer& scratch, int32_t* D, int64_t* I,
                        hipStream_t s) {
    if (n <= 0) return;
    bn_check(n, d, k);
    FAISS_THROW_IF_NOT_MSG(ntotal < ((int64_t)1 << 32), "binary_flat_search: ntotal must be < 2^32");
    BinArgs g;
    g.W = (d + 31) / 32;
    g.k = k;
    g.codes = codes;
    g.ntotal = ntotal;
    const bool dense = k > BIN_KSEL;
    const int64_t rows = std::max<int64_t>(ntotal, 1);
    // queries per work group: 16, or 8 when the tile of 16 and its candidate
    // buffers exceed the LDS (d > 48640 bits with k <= BIN_KSEL: 64 + 32 KiB at
    // d = 65536)
    const int QT = bn_lds(BN_QT, 4, g.W, !dense) <= BN_LDS_MAX ? BN_QT : BN_QT / 2;
    // queries of one launch, by the scratch
    int64_t qc = std::min<int64_t>(n, (int64_t)1 << 20);
    if (dense) qc = std::min<int64_t>(qc, std::max<int64_t>(1, BN_SCRATCH / (4 * rows)));
    const int64_t groups_max = (int64_t)cdiv((size_t)qc, (size_t)QT);
    // slabs: fill the chip when the batch is small, none shorter than 1024 rows
    int64_t nslab = std::max<int64_t>(
            1, std::min<int64_t>((int64_t)cdiv(1024, (size_t)groups_max), rows / 1024));
    g.slab_rows = (int64_t)roundup(cdiv((size_t)rows, (size_t)nslab), 256);
    nslab = (int64_t)cdiv((size_t)rows, (size_t)g.slab_rows);
    g.PC = 2 * k;
    g.nparts = (int)nslab * 4;
    const int64_t k_base = (int64_t)g.nparts * g.PC;
    if (!dense) qc = std::min<int64_t>(qc, std::max<int64_t>(1, BN_SCRATCH / (12 * k_base)));
    if (dense) {
        scratch.reserve(sizeof(float) * (size_t)qc * rows);
        g.dense = scratch.as<float>();
    } else {
        scratch.reserve((sizeof(uint32_t) + sizeof(int64_t)) * (size_t)qc * k_base);
        g.plabels = scratch.as<int64_t>();
        g.pkeys = (uint32_t*)(g.plabels + qc * k_base);
    }
    for (int64_t q = 0; q < n; q += qc) {
        g.x = x + q * g.W;
        g.n = std::min(qc, n - q);
        float* Df = (float*)(D + q * k);
        const int64_t groups = (int64_t)cdiv((size_t)g.n, (size_t)QT);
        if (ntotal > 0 && QT == BN_QT) bn_launch<BN_QT, 4, false>(g, groups, nslab, s);
        else if (ntotal > 0) bn_launch<BN_QT / 2, 4, false>(g, groups, nslab, s);
        if (dense) {
            // (no rows: the select over zero columns pads every slot)
            select_rows_exact<int64_t>(g.dense, g.n, ntotal, ntotal, k, 1, 0, Df, I + q * k, k, s);
        } else {
            if (ntotal == 0) {
                k_bin_fill<<<stride_grid(g.n * k_base, 256), dim3(256), 0, s>>>(
                        g.pkeys, g.plabels, g.n * k_base);
                HIP_LAUNCH_CHECK();
            }
            refine_select(g.pkeys, g.plabels, g.n, k_base, k, 1, Df, I + q * k, s);
        }
        k_bin_finish<<<stride_grid(g.n * k, 256), dim3(256), 0, s>>>(
                D + q * k, I + q * k, g.n, k, 0, nullptr, 0, nullptr, nullptr);
        HIP_LAUNCH_CHECK();
    }
}

void binary_probes(const int64_t* coarse, int64_t n, int np, const uint32_t* list_len, int nlist,
                   int64_t max_codes, int32_t* assign, hipStream_t s) {
    if (n <= 0 || np <= 0) return;
    k_bin_probes<<<stride_grid(n, 256), dim3(256), 0, s>>>(coarse, n, np, list_len, nlist,
                                                           max_codes, assign);
    HIP_LAUNCH_CHECK();
}

void binary_ivf_scan(const uint32_t* x, int64_t n, int d, const uint32_t* codes,
                     const int64_t* ids, const int64_t* list_off, const uint32_t* list_len,
                     uint32_t max_list_len, const int32_t* assign, int np, int k, bool use_heap,
                     DeviceBuffer& scratch, int32_t* D, int64_t* I, hipStream_t s) {
    if (n <= 0) return;
    bn_check(n, d, k);
    FAISS_THROW_IF_NOT_FMT(np >= 1 && np <= 65535, "nprobe = %d must be in [1, 65535]", np);
    BinArgs g;
    g.W = (d + 31) / 32;
    g.k = k;
    g.codes = codes;
    g.ids = ids;
    g.list_off = list_off;
    g.list_len = list_len;
    g.np = np;
    g.by_pos = use_heap ? 0 : 1;
    const bool dense = k > BIN_KSEL;
    const bool wide = max_list_len > 1024;  // four waves per (query, probe)
    g.PC = 2 * k;
    g.nparts = np * (wide ? 4 : 1);
    g.maxlen = std::max<int64_t>(max_list_len, 1);
    g.cap = std::max<int64_t>((int64_t)np * g.maxlen, k);
    const int64_t k_base = dense ? g.cap : (int64_t)g.nparts * g.PC;
    FAISS_THROW_IF_NOT_FMT(12 * (size_t)k_base <= ((size_t)4 << 30),
                           "binary_ivf_scan: k = %d > %d with nprobe = %d and a list of %u rows "
                           "needs a candidate table of %zu bytes per query",
                           k, BIN_KSEL, np, max_list_len, 12 * (size_t)k_base);
    const int64_t qc = std::max<int64_t>(
            1, std::min<int64_t>(std::min<int64_t>(n, (int64_t)1 << 20),
                                 (int64_t)(BN_SCRATCH / (12 * (size_t)k_base))));
    scratch.reserve(12 * (size_t)qc * k_base);
    int64_t* labels = scratch.as<int64_t>();
    uint32_t* keys = (uint32_t*)(labels + qc * k_base);
    if (dense) {
        g.ckeys = keys;
        g.clabels = labels;
    } else {
        g.pkeys = keys;
        g.plabels = labels;
    }
    for (int64_t q = 0; q < n; q += qc) {
        g.x = x + q * g.W;
        g.n = std::min(qc, n - q);
        g.assign = assign + q * np;
        if (dense) {
            k_bin_fill<<<stride_grid(g.n * k_base, 256), dim3(256), 0, s>>>(keys, labels,
                                                                            g.n * k_base);
            HIP_LAUNCH_CHECK();
        }
        if (wide) bn_launch<1, 4, true>(g, g.n, np, s);
        else bn_launch<1, 1, true>(g, g.n, np, s);
        refine_select(keys, labels, g.n, k_base, k, 1, (float*)(D + q * k), I + q * k, s);
        k_bin_finish<<<stride_grid(g.n * k, 256), dim3(256), 0, s>>>(
                D + q * k, I + q * k, g.n, k, g.by_pos, g.assign, np, list_off, ids);
        HIP_LAUNCH_CHECK();
    }
}

}  // namespace kern
}  // namespace faiss_amd
