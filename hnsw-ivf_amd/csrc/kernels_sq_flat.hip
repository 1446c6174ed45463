// kernels_sq_flat.hip — IndexScalarQuantizer's full scan: exact distances of a
// batch of queries to every row of a flat array of SQ8 / SQfp16 codes, each
// code decoded once per tile of 64 queries.
//
// Reference behaviour: faiss/IndexScalarQuantizer.cpp:48-90 runs the inverted
// list scanner of faiss/impl/ScalarQuantizer.cpp over the whole code array
// (scan_codes, store_pairs, list 0), i.e. the 8-wide DCTemplate whose fp32
// evaluation order csrc/sq_ref.h states.  Every arithmetic step below is a
// function of that header; nothing is restated.
//
// Geometry.  A 256-thread group owns SF_Q = 64 queries x SF_R = 64 rows and
// walks d in slices of SF_DS = 32 components; consecutive groups walk the row
// tiles of one query tile.  Thread (tx = t & 15, ty = t >> 4) keeps the 4 x 4
// pairs of queries 4 ty + a and rows tx + 16 b, eight lane accumulators each
// (component j feeds lane j & 7, as SimilarityL2<8> / SimilarityIP<8>), and
// finishes a pair with sq_reduce8.
//
// Decode once, on the way into LDS.  The codes leave HBM as raw bytes: thread
// t stages the 8 components (t & 3) * 8 .. + 7 of row t >> 2 of the slice, one
// 8-byte load for SQ8 (a row pitch of d bytes with d % 8 == 0 allows no more:
// d = 72), one 16-byte load for fp16 (pitch 2 d, always 16-byte aligned).  The
// same thread holds vmin / vdiff of its 8 components (two float4 each, read
// with the codes), turns the codes into the fp32 reconstructions with
// sq_recons8 / sq_half_to_float and stores two float4 in LDS.  The 64 queries
// of the tile then reuse each decoded component: the inner loop is a plain
// fp32 one, `t = y - x^; acc = fmaf(t, t, acc)` for L2 and one fmaf for the
// inner product.  The next slice's global loads (codes, ranges, queries) are
// issued before the current slice is evaluated and land in LDS after it.
//
// LDS.  Both operands at a pitch of SF_P = 36 words per row of a slice: the 16
// threads of a wave that read 16 different rows with one ds_read_b128 start
// 36 tx mod 64 words apart, sixteen disjoint groups of four banks; the four
// query addresses of a wave are broadcasts.  2 x 64 x 36 x 4 = 18 KiB.
//
// Edges.  Rows >= ntotal and queries >= nq are staged as zeros and never
// stored; components >= d of the last slice are staged as zeros and never
// evaluated (d % 8 == 0, so the loop over 8-component groups stops at d).  A
// row the selector excludes gets the key the select never admits (+inf for
// L2, -inf for the inner product), as IndexFlat's selected search does.
//
// Output.  Dense distance rows [nq][ntotal] of a chunk of queries in scratch
// (256 MiB at most), then select_rows_exact (the reference heap's result,
// arrival-order ties).  No host round trip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "sq_ref.h"

namespace faiss_amd {
namespace kern {

namespace {

constexpr int SF_Q = 64, SF_R = 64, SF_DS = 32, SF_P = SF_DS + 4;

// the raw codes of 8 components of one row, and for SQ8 their ranges
template <int QT>
struct CodeRegs;
template <>
struct CodeRegs<SQ_QT_8bit> {
    uint2 c;
    float4 vmin[2], vdiff[2];
};
template <>
struct CodeRegs<SQ_QT_fp16> {
    uint4 c;
};

__device__ __forceinline__ CodeRegs<SQ_QT_8bit> load_codes(
        std::integral_constant<int, SQ_QT_8bit>, const uint8_t* __restrict__ codes,
        const float* __restrict__ trained, int64_t row, int64_t ntotal, int k, int d) {
    CodeRegs<SQ_QT_8bit> r;
    r.c = make_uint2(0u, 0u);
    r.vmin[0] = r.vmin[1] = r.vdiff[0] = r.vdiff[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < ntotal && k < d) {  // k % 8 == 0, d % 8 == 0: 8 bytes inside the row
        r.c = *(const uint2*)(codes + row * d + k);
        r.vmin[0] = *(const float4*)(trained + k);
        r.vmin[1] = *(const float4*)(trained + k + 4);
        r.vdiff[0] = *(const float4*)(trained + d + k);
        r.vdiff[1] = *(const float4*)(trained + d + k + 4);
    }
    return r;
}
__device__ __forceinline__ CodeRegs<SQ_QT_fp16> load_codes(
        std::integral_constant<int, SQ_QT_fp16>, const uint8_t* __restrict__ codes,
        const float* __restrict__, int64_t row, int64_t ntotal, int k, int d) {
    CodeRegs<SQ_QT_fp16> r;
    r.c = make_uint4(0u, 0u, 0u, 0u);
    if (row < ntotal && k < d)  // 16 bytes inside the row of 2 d bytes
        r.c = *(const uint4*)(codes + (row * d + k) * 2);
    return r;
}

// codes -> the 8 fp32 reconstructions (zeros for a padding row or dimension:
// the zero ranges / the zero half)
__device__ __forceinline__ void decode8(const CodeRegs<SQ_QT_8bit>& r, float4& lo, float4& hi) {
    lo.x = sq_recons8((uint8_t)(r.c.x), r.vmin[0].x, r.vdiff[0].x);
    lo.y = sq_recons8((uint8_t)(r.c.x >> 8), r.vmin[0].y, r.vdiff[0].y);
    lo.z = sq_recons8((uint8_t)(r.c.x >> 16), r.vmin[0].z, r.vdiff[0].z);
    lo.w = sq_recons8((uint8_t)(r.c.x >> 24), r.vmin[0].w, r.vdiff[0].w);
    hi.x = sq_recons8((uint8_t)(r.c.y), r.vmin[1].x, r.vdiff[1].x);
    hi.y = sq_recons8((uint8_t)(r.c.y >> 8), r.vmin[1].y, r.vdiff[1].y);
    hi.z = sq_recons8((uint8_t)(r.c.y >> 16), r.vmin[1].z, r.vdiff[1].z);
    hi.w = sq_recons8((uint8_t)(r.c.y >> 24), r.vmin[1].w, r.vdiff[1].w);
}
__device__ __forceinline__ void decode8(const CodeRegs<SQ_QT_fp16>& r, float4& lo, float4& hi) {
    lo.x = sq_half_to_float((uint16_t)(r.c.x));
    lo.y = sq_half_to_float((uint16_t)(r.c.x >> 16));
    lo.z = sq_half_to_float((uint16_t)(r.c.y));
    lo.w = sq_half_to_float((uint16_t)(r.c.y >> 16));
    hi.x = sq_half_to_float((uint16_t)(r.c.z));
    hi.y = sq_half_to_float((uint16_t)(r.c.z >> 16));
    hi.z = sq_half_to_float((uint16_t)(r.c.w));
    hi.w = sq_half_to_float((uint16_t)(r.c.w >> 16));
}

// this thread's two float4 of the query slice; zeros for queries >= nq, dims >= d
__device__ __forceinline__ float4 load_query(const float* __restrict__ x, int64_t row, int64_t nq,
                                             int ldx, int k, int d) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nq && k < d) v = *(const float4*)(x + row * ldx + k);  // k % 4 == 0, d % 8 == 0
    return v;
}

template <bool L2, int QT>
__global__ __launch_bounds__(256, 2) void k_sq_flat(
        const float* __restrict__ x, int64_t nq, int ldx, const uint8_t* __restrict__ codes,
        int64_t ntotal, const float* __restrict__ trained, int d,
        const uint8_t* __restrict__ mask, float* __restrict__ D, int64_t ldD, int tiles_r) {
    using QTag = std::integral_constant<int, QT>;
    __shared__ float Xs[SF_Q * SF_P];
    __shared__ float Ys[SF_R * SF_P];
    const int t = threadIdx.x;
    const int tx = t & 15, ty = t >> 4;
    const int64_t q0 = (int64_t)(blockIdx.x / tiles_r) * SF_Q;
    const int64_t r0 = (int64_t)(blockIdx.x % tiles_r) * SF_R;
    // staging roles: queries sq (+32), float4 column sqc; code row sr, components src .. + 7
    const int sq = t >> 3, sqc = (t & 7) * 4;
    const int sr = t >> 2, src = (t & 3) * 8;

    float acc[4][4][8];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int j = 0; j < 8; j++) acc[a][b][j] = 0.f;

    struct SliceRegs {
        float4 x[2];
        CodeRegs<QT> y;
    };
    auto fetch = [&](int k0) {
        SliceRegs r;
        r.x[0] = load_query(x, q0 + sq, nq, ldx, k0 + sqc, d);
        r.x[1] = load_query(x, q0 + sq + 32, nq, ldx, k0 + sqc, d);
        r.y = load_codes(QTag{}, codes, trained, r0 + sr, ntotal, k0 + src, d);
        return r;
    };
    auto stage = [&](const SliceRegs& r) {
        *(float4*)(Xs + sq * SF_P + sqc) = r.x[0];
        *(float4*)(Xs + (sq + 32) * SF_P + sqc) = r.x[1];
        float4 lo, hi;
        decode8(r.y, lo, hi);
        *(float4*)(Ys + sr * SF_P + src) = lo;
        *(float4*)(Ys + sr * SF_P + src + 4) = hi;
    };
    const float* xs = Xs + 4 * ty * SF_P;
    const float* ys = Ys + tx * SF_P;
    // four components at slice offset k into lanes J0 .. J0 + 3
    auto step4 = [&](int k, auto j0) {
        constexpr int J0 = decltype(j0)::value;
        float4 xv[4], yv[4];
#pragma unroll
        for (int a = 0; a < 4; a++) xv[a] = *(const float4*)(xs + a * SF_P + k);
#pragma unroll
        for (int b = 0; b < 4; b++) yv[b] = *(const float4*)(ys + 16 * b * SF_P + k);
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                float* c = acc[a][b];
                c[J0] = sq_acc<L2>(xv[a].x, yv[b].x, c[J0]);
                c[J0 + 1] = sq_acc<L2>(xv[a].y, yv[b].y, c[J0 + 1]);
                c[J0 + 2] = sq_acc<L2>(xv[a].z, yv[b].z, c[J0 + 2]);
                c[J0 + 3] = sq_acc<L2>(xv[a].w, yv[b].w, c[J0 + 3]);
            }
    };
    using I0 = std::integral_constant<int, 0>;
    using I4 = std::integral_constant<int, 4>;

    const int nslice = (d + SF_DS - 1) / SF_DS;
    SliceRegs nxt = fetch(0);
    for (int sl = 0; sl < nslice; sl++) {
        const int k0 = sl * SF_DS;
        __syncthreads();  // the previous slice has been read
        stage(nxt);
        __syncthreads();
        if (sl + 1 < nslice) nxt = fetch(k0 + SF_DS);
        const int kb = min(SF_DS, d - k0);  // a multiple of 8
#pragma unroll 2
        for (int k = 0; k < kb; k += 8) {
            step4(k, I0{});
            step4(k + 4, I4{});
        }
    }
    const float excluded = L2 ? HUGE_VALF : -HUGE_VALF;
    bool member[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int64_t col = r0 + tx + 16 * b;
        member[b] = col < ntotal && (!mask || mask[col]);
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int64_t row = q0 + 4 * ty + a;
        if (row >= nq) continue;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int64_t col = r0 + tx + 16 * b;
            if (col < ntotal) D[row * ldD + col] = member[b] ? sq_reduce8(acc[a][b]) : excluded;
        }
    }
}

template <bool L2, int QT>
void launch_sq_flat(const SQFlatArgs& a, const float* x, int64_t nq, float* dense, hipStream_t s) {
    const int64_t tq = (int64_t)cdiv((size_t)nq, SF_Q), tr = (int64_t)cdiv((size_t)a.ntotal, SF_R);
    FAISS_THROW_IF_NOT(tr < (1ll << 31) && tq * tr < (1ll << 31));
    k_sq_flat<L2, QT><<<kgrid(tq * tr, 256), dim3(256), 0, s>>>(
            x, nq, a.ldx, a.codes, a.ntotal, a.trained, a.d, a.mask, dense, a.ntotal, (int)tr);
    HIP_LAUNCH_CHECK();
}

}  // namespace

int64_t sq_flat_query_chunk(int64_t n, int64_t ntotal) {
    // 256 MiB of dense rows (IndexFlat::search_extra_metric's budget); whole
    // query tiles where more than one fits
    int64_t qc = ((int64_t)1 << 26) / std::max<int64_t>(ntotal, 1);
    if (qc >= SF_Q) qc = qc / SF_Q * SF_Q;
    return std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(n, 1), qc));
}

void sq_flat_search(const SQFlatArgs& a, DeviceBuffer& s_dense, DeviceBuffer& s_sel, float* D,
                    int64_t* I, hipStream_t s, KernelTimes* kt) {
    FAISS_THROW_IF_NOT(a.qtype == SQ_QT_8bit || a.qtype == SQ_QT_fp16);
    FAISS_THROW_IF_NOT(a.d >= 8 && a.d % 8 == 0 && a.ldx % 4 == 0 && a.ldx >= a.d);
    FAISS_THROW_IF_NOT(a.k >= 1 && a.k <= kMaxKExact && a.ntotal >= 0);
    FAISS_THROW_IF_NOT(a.ntotal == 0 || (a.codes && (a.qtype == SQ_QT_fp16 || a.trained)));
    if (a.n <= 0) return;
    const int64_t ny = std::max<int64_t>(a.ntotal, 1);
    const int64_t qc = sq_flat_query_chunk(a.n, a.ntotal);
    s_dense.reserve(sizeof(float) * (size_t)qc * (size_t)ny);
    float* dense = s_dense.as<float>();
    for (int64_t q0 = 0; q0 < a.n; q0 += qc) {
        const int64_t nq = std::min(qc, a.n - q0);
        const float* x = a.x + q0 * a.ldx;
        if (a.ntotal > 0) {
            ScopedKernelTimer tm(kt, "sq_flat_scan", 0.0, s);
            if (a.qtype == SQ_QT_8bit) {
                if (a.l2)
                    launch_sq_flat<true, SQ_QT_8bit>(a, x, nq, dense, s);
                else
                    launch_sq_flat<false, SQ_QT_8bit>(a, x, nq, dense, s);
            } else {
                if (a.l2)
                    launch_sq_flat<true, SQ_QT_fp16>(a, x, nq, dense, s);
                else
                    launch_sq_flat<false, SQ_QT_fp16>(a, x, nq, dense, s);
            }
        }
        ScopedKernelTimer tm(kt, "sq_flat_select", 0.0, s);
        select_rows_exact<int64_t>(dense, nq, a.ntotal, a.ntotal, a.k, a.l2, 0, D + q0 * a.k,
                                   I + q0 * a.k, a.k, s, &s_sel);
    }
}

}  // namespace kern
}  // namespace faiss_amd
