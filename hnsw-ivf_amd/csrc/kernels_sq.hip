// kernels_sq.hip — the exact IVF scan of scalar-quantizer codes (SQ8, SQfp16).
//
// Reference hot loop: IVFSQScannerL2 / IVFSQScannerIP::scan_codes over
// DCTemplate<Quantizer, Similarity, 8>::query_to_code
// (faiss/impl/ScalarQuantizer.cpp:2121-2296, :1930-2020), restated in sq_ref.h.
//
// k_ex_sq has the contract of k_ex_flat / k_ex_pq (kernels_exact.hip): for
// every (query, probe) it writes ex_key(dis) and the arena row of each scanned
// row in arrival order at q * cap + eoff[e]; rows outside the selector get
// EX_SKIP; `lim` cuts the list (max_codes).  k_ex_select then runs unchanged.
//
// Shape: one 256-thread workgroup per (query, probe).  The query side y (the
// residual x - centroid for L2 by residual, else x) and vmin / vdiff are staged
// once in LDS (3 d floats); every thread then owns one row: it reads the code
// row 16 bytes per load (rows start at multiples of the 16-byte padded stride)
// and keeps the reference's eight lane accumulators in registers.  All threads
// read the same LDS address at the same time (a broadcast, no bank conflicts).
// Per component: SQ8 one load byte, a convert, two fma (decode, reconstruct), a
// subtract and an fma (L2); fp16 a convert, a subtract and an fma.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "common.h"
#include "kernels.h"
#include "sq_ref.h"
#include "wave_select.h"

namespace faiss_amd {
namespace kern {

namespace {

// threads per (query, probe) workgroup.  Measured on the IVF4096,SQ8 d = 128
// shape of scripts/exp_sq_scan.py (lists of ~315 rows): scan stage 4.72 ms per
// step with 256, 5.60 ms with 128, 8.95 ms with 64 -- the staging of y / vmin /
// vdiff and its barrier are paid per workgroup, so fewer, larger groups win
// although the last pass over a list leaves more threads idle.
constexpr int SQ_TPB = 256;

// eight components j0 .. j0 + 7 (j0 % 8 == 0) of one row into acc[0..8)
template <bool L2, int QT>
__device__ __forceinline__ void sq_acc8(const float* __restrict__ ys, const float* __restrict__ vmin,
                                        const float* __restrict__ vdiff, int j0, uint32_t w0,
                                        uint32_t w1, uint32_t w2, uint32_t w3, float (&acc)[8]) {
    const float4 ya = *(const float4*)(ys + j0), yb = *(const float4*)(ys + j0 + 4);
    const float y[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
    float xr[8];
    if (QT == SQ_QT_fp16) {
        const uint32_t w[4] = {w0, w1, w2, w3};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            xr[2 * i] = sq_half_to_float((uint16_t)(w[i] & 0xffffu));
            xr[2 * i + 1] = sq_half_to_float((uint16_t)(w[i] >> 16));
        }
    } else {
        const float4 ma = *(const float4*)(vmin + j0), mb = *(const float4*)(vmin + j0 + 4);
        const float4 da = *(const float4*)(vdiff + j0), db = *(const float4*)(vdiff + j0 + 4);
        const float m[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
        const float dv[8] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w};
        const uint32_t w[2] = {w0, w1};
#pragma unroll
        for (int i = 0; i < 8; i++)
            xr[i] = sq_recons8((uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 0xffu), m[i], dv[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = sq_acc<L2>(y[i], xr[i], acc[i]);
}

template <bool L2, int QT>
__global__ __launch_bounds__(SQ_TPB) void k_ex_sq(const float* __restrict__ x, int ldx, int d, int np,
                                               const int32_t* __restrict__ assign,
                                               const float* __restrict__ cdis,
                                               const uint32_t* __restrict__ lim,
                                               const uint32_t* __restrict__ list_off,
                                               const uint32_t* __restrict__ list_len, int nlist,
                                               ExactSQ sq, const uint8_t* __restrict__ sel,
                                               const uint32_t* __restrict__ eoff, int64_t cap,
                                               uint32_t* __restrict__ okeys,
                                               uint32_t* __restrict__ orows, int64_t e0) {
    extern __shared__ float sq_lds[];  // ys [d] | vmin [d] | vdiff [d]
    const int64_t e = e0 + blockIdx.x;
    const int64_t q = e / np;
    const int32_t key = assign[e];
    if (key < 0 || key >= nlist) return;
    const uint32_t len = lim ? lim[e] : list_len[key];
    if (len == 0) return;
    float* ys = sq_lds;
    float* vmin = ys + d;
    float* vdiff = vmin + d;
    // IVFSQScannerL2::set_list: Index::compute_residual, one rounded subtract
    const bool resid = L2 && sq.by_residual;
    const float* xq = x + q * ldx;
    const float* yc = sq.cent + (int64_t)key * sq.ldcent;
    for (int i = threadIdx.x; i < d; i += SQ_TPB) {
        ys[i] = resid ? xq[i] - yc[i] : xq[i];
        if (QT == SQ_QT_8bit) {
            vmin[i] = sq.trained[i];
            vdiff[i] = sq.trained[d + i];
        }
    }
    __syncthreads();
    // IVFSQScannerIP::set_list: accu0 = coarse_dis when by residual
    const float accu0 = (!L2 && sq.by_residual && cdis) ? cdis[e] : 0.f;
    const uint32_t off = list_off[key];
    const int64_t base = q * cap + eoff[e];
    const int row_bytes = QT == SQ_QT_fp16 ? 2 * d : d;
    for (uint32_t r = threadIdx.x; r < len; r += SQ_TPB) {
        const uint32_t row = off + r;
        uint32_t k = EX_SKIP;
        if (!sel || sel[row]) {
            const uint4* cp = (const uint4*)(sq.codes + (int64_t)row * sq.cs);
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            // 16 bytes per load: 16 SQ8 components or 8 halves; the stride is
            // padded to 16 bytes, so the last load of a d % 16 == 8 SQ8 row
            // stays inside the row's slot
            for (int b = 0; b < row_bytes; b += 16) {
                const uint4 c = cp[b >> 4];
                if (QT == SQ_QT_fp16) {
                    sq_acc8<L2, QT>(ys, vmin, vdiff, b >> 1, c.x, c.y, c.z, c.w, acc);
                } else {
                    sq_acc8<L2, QT>(ys, vmin, vdiff, b, c.x, c.y, 0u, 0u, acc);
                    if (b + 8 < row_bytes)
                        sq_acc8<L2, QT>(ys, vmin, vdiff, b + 8, c.z, c.w, 0u, 0u, acc);
                }
            }
            const float s = sq_reduce8(acc);
            k = ex_key(L2 ? s : accu0 + s, L2);
        }
        okeys[base + r] = k;
        orows[base + r] = row;
    }
}

}  // namespace

void ivf_exact_sq_scan(const ExactScanArgs& a, const uint32_t* eoff, int64_t cap, uint32_t* keys,
                       uint32_t* rows, hipStream_t s) {
    const ExactSQ& sq = a.sq;
    FAISS_THROW_IF_NOT_FMT(sq.qtype == SQ_QT_8bit || sq.qtype == SQ_QT_fp16,
                           "IndexIVFScalarQuantizer: qtype %d has no scan kernel", sq.qtype);
    // (every 16-byte load of a row stays inside its slot)
    const bool shape_ok = (a.d & 7) == 0 && (sq.cs & 15) == 0 &&
                          sq.cs >= (sq.qtype == SQ_QT_fp16 ? 2 : 1) * a.d;
    FAISS_THROW_IF_NOT_FMT(shape_ok,
                           "IndexIVFScalarQuantizer: d = %d, code stride %d not scannable", a.d,
                           sq.cs);
    const size_t lds = sizeof(float) * 3 * (size_t)a.d;
    FAISS_THROW_IF_NOT_FMT(lds <= 64 * 1024, "IndexIVFScalarQuantizer: d = %d too large", a.d);
    const int64_t entries = a.n * (int64_t)a.np;
    constexpr int64_t per_launch = (int64_t)1 << 20;
#define EXSQ(L2, QT)                                                                         \
    k_ex_sq<L2, QT><<<kgrid(ne, SQ_TPB), dim3(SQ_TPB), lds, s>>>(                            \
            a.x, a.ldx, a.d, a.np, a.assign, a.cdis, a.lim, a.list_off, a.list_len, a.nlist, \
            sq, a.sel, eoff, cap, keys, rows, e0)
    for (int64_t e0 = 0; e0 < entries; e0 += per_launch) {
        const int64_t ne = std::min(per_launch, entries - e0);
        if (sq.qtype == SQ_QT_8bit) {
            if (a.l2)
                EXSQ(true, SQ_QT_8bit);
            else
                EXSQ(false, SQ_QT_8bit);
        } else {
            if (a.l2)
                EXSQ(true, SQ_QT_fp16);
            else
                EXSQ(false, SQ_QT_fp16);
        }
    }
#undef EXSQ
    HIP_LAUNCH_CHECK();
}

}  // namespace kern
}  // namespace faiss_amd
