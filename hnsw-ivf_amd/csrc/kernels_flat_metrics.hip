// kernels_flat_metrics.hip — IndexFlat's other metrics as a VALU tile kernel.
//
// Reference behaviour: faiss/utils/extra_distances-inl.h (VectorDistance<mt>)
// under knn_extra_metrics (faiss/utils/extra_distances.cpp:55-96): one
// distance per (query, row), evaluated in a fixed order over the dimensions.
// None of the nine metrics is a contraction, so the MFMA tile of flat_tile.h
// does not apply; this tile runs on the vector ALU.
//
// Geometry.  A 256-thread group owns MT_Q = 64 queries x MT_R = 64 rows.  Both
// operands go through the LDS in slices of MT_DS = 32 dimensions, a row of a
// slice at a pitch of MT_P = 36 words: the 16 threads of a wave that read 16
// different rows with one ds_read_b128 then start 36 tx mod 64 words apart,
// sixteen disjoint groups of four banks.  Thread (tx = t & 15, ty = t >> 4)
// keeps the 4 x 4 pairs of queries 4 ty + a and rows tx + 16 b in registers
// (a wave's stores of one (a, b) cover 16 consecutive columns of D).  The next
// slice's global loads (16-byte, two per operand and thread) are issued before
// the current slice is evaluated and land in the LDS after it.
//
// Evaluation order, per pair, independent of the pair's place in the tile:
//  * L1, Linf (fvec_L1 / fvec_Linf, the AVX2 branch of
//    faiss/utils/distances_simd.cpp:2590-2674): eight lane accumulators over
//    the dims 8 m + j < n8 = d & ~7; lanes j + 4 and j combined into four;
//    one 4-wide step if d - n8 >= 4; one masked step over the last d % 4 dims
//    (the other lanes take |0 - 0|); then (c0 + c1) + (c2 + c3), for Linf
//    max(max(c2, c0), max(c3, c1)).  The maximum is the SSE one, a > b ? a : b.
//    8 lanes x 16 pairs = 128 accumulators: the widest instantiation.
//  * the others: the plain loop over i = 0 .. d - 1 of extra_distances-inl.h.
//    NaNEuclidean's `accu += diff * diff` is one fused multiply-add: the
//    reference build is g++ -O3 -mfma with GCC's default -ffp-contract=fast,
//    which contracts the expression (the conditional float reduction is not
//    vectorised without -ffast-math, so the order stays i = 0 .. d - 1).
//    ABS_INNER_PRODUCT's fabs sits between its product and its sum: not fused.
//    The reference calls the C `fabs`, `fmin`, `fmax` and `log`, which take
//    doubles.  That changes no bit where a double result of float operands
//    is rounded to float at once (53 >= 2 x 24 + 2 bits), but Canberra's
//    denominator, quotient and accumulation stay in double, one rounding per
//    term, and so they do here.
//  * Lp and JensenShannon call the device powf / log (double, as the
//    reference's); the seven others use IEEE basic operations only (this library is built with -ffp-contract=off
//    and hipcc's correctly rounded fp32 division).
// Dimensions >= d are never evaluated by the plain loops (a zero pad would
// give Canberra 0 / 0); the staging writes zeros there whatever the operands'
// padding holds.  Rows and queries beyond ny / nx are neither read nor written.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "kernels.h"

namespace faiss_amd {
namespace kern {

namespace {

constexpr int MT_Q = 64, MT_R = 64, MT_DS = 32, MT_P = MT_DS + 4;

// faiss/MetricType.h
constexpr int M_L1 = 2, M_Linf = 3, M_Lp = 4, M_Canberra = 20, M_BrayCurtis = 21,
              M_JensenShannon = 22, M_Jaccard = 23, M_NaNEuclidean = 24, M_AbsIP = 25;

// _mm_max_ps(a, b)
__device__ __forceinline__ float sse_max(float a, float b) { return a > b ? a : b; }

// Per-pair state of metric MT.  LANES == 8: add<J> feeds lane J (dims 8 m + J,
// after fold() the 4-wide lanes); LANES == 1: add<J> feeds the one chain.
template <int MT>
struct MetricOp {
    static constexpr int LANES = (MT == M_L1 || MT == M_Linf) ? 8 : 1;
    static constexpr bool LIBM = MT == M_Lp || MT == M_JensenShannon;
    static constexpr bool TWO = MT == M_BrayCurtis || MT == M_Jaccard || MT == M_NaNEuclidean;
    float c[LANES];
    float e[1];  // second sum (denominator / present count) of the TWO metrics

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < LANES; j++) c[j] = 0.f;
        e[0] = 0.f;
    }
    template <int J>
    __device__ __forceinline__ void add(float x, float y, float arg) {
        constexpr int L = LANES == 8 ? J : 0;
        if (MT == M_L1) {
            c[L] = c[L] + fabsf(x - y);
        } else if (MT == M_Linf) {
            c[L] = sse_max(c[L], fabsf(x - y));
        } else if (MT == M_Lp) {
            c[L] += powf(fabsf(x - y), arg);
        } else if (MT == M_Canberra) {
            // the reference's `fabs` is the double one: float difference,
            // then the sum of the magnitudes, the quotient and the
            // accumulation in double, rounded to float once per term
            // (pinned by tests/golden/flat_metrics_ref.npz)
            const double q = fabs((double)(x - y)) / ((double)fabsf(x) + (double)fabsf(y));
            c[L] = (float)((double)c[L] + q);
        } else if (MT == M_BrayCurtis) {
            c[L] += fabsf(x - y);
            e[0] += fabsf(x + y);
        } else if (MT == M_JensenShannon) {
            const float mi = 0.5f * (x + y);
            // the reference's `log` is the double one (no float overload of
            // ::log in scope): float quotient, double log and product, one
            // rounding to float.  In float the rounding of mi / x alone would
            // cost a nearest neighbour's distance several per cent.
            const float kl1 = (float)(-(double)x * log((double)(mi / x)));
            const float kl2 = (float)(-(double)y * log((double)(mi / y)));
            c[L] += kl1 + kl2;
        } else if (MT == M_Jaccard) {
            c[L] += fminf(x, y);
            e[0] += fmaxf(x, y);
        } else if (MT == M_NaNEuclidean) {
            if (!(x != x) && !(y != y)) {
                const float diff = x - y;
                c[L] = fmaf(diff, diff, c[L]);
                e[0] += 1.f;  // exact below 2^24 dims
            }
        } else {
            c[L] += fabsf(x * y);
        }
    }
    // 8 lanes -> 4: extractf128(1) op extractf128(0)
    __device__ __forceinline__ void fold() {
        if constexpr (LANES == 8) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                c[j] = MT == M_Linf ? sse_max(c[j + 4], c[j]) : c[j + 4] + c[j];
        }
    }
    __device__ __forceinline__ float finish(int d) const {
        constexpr int W = LANES == 8 ? 1 : 0;  // (indices stay in bounds for LANES == 1)
        if (MT == M_L1) return (c[0] + c[W]) + (c[2 * W] + c[3 * W]);
        if (MT == M_Linf) {
            const float t0 = sse_max(c[2 * W], c[0]), t1 = sse_max(c[3 * W], c[W]);
            return sse_max(t0, t1);
        }
        if (MT == M_BrayCurtis || MT == M_Jaccard) return c[0] / e[0];
        if (MT == M_JensenShannon) return 0.5f * c[0];
        if (MT == M_NaNEuclidean) {
            if (e[0] == 0.f) return NAN;
            return (float)d / e[0] * c[0];
        }
        return c[0];
    }
};

// global -> registers: this thread's two float4 of each operand's slice at
// dims [k0, k0 + MT_DS); zeros for rows >= n and dims >= d
struct SliceRegs {
    float4 x[2], y[2];
};
__device__ __forceinline__ float4 load_masked(const float* __restrict__ base, int64_t row,
                                              int64_t n, int ld, int k, int d) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n && k < d) {  // k < d <= ld, k % 4 == 0, ld % 4 == 0: 16 bytes inside the row
        v = *(const float4*)(base + row * ld + k);
        if (k + 1 >= d) v.y = 0.f;
        if (k + 2 >= d) v.z = 0.f;
        if (k + 3 >= d) v.w = 0.f;
    }
    return v;
}

template <int MT>
__global__ __launch_bounds__(256, 2) void k_metric_tile(const float* __restrict__ x, int64_t nx,
                                                        int ldx, const float* __restrict__ y,
                                                        int64_t ny, int ldy, int d, float arg,
                                                        float* __restrict__ D, int64_t ldD,
                                                        int tiles_y) {
    using Op = MetricOp<MT>;
    __shared__ float Xs[MT_Q * MT_P];
    __shared__ float Ys[MT_R * MT_P];
    const int t = threadIdx.x;
    const int tx = t & 15, ty = t >> 4;
    // consecutive blocks walk the row tiles of one query tile
    const int64_t q0 = (int64_t)(blockIdx.x / tiles_y) * MT_Q;
    const int64_t r0 = (int64_t)(blockIdx.x % tiles_y) * MT_R;
    // staging role: row sr (+32), float4 column sc of the slice
    const int sr = t >> 3, sc = (t & 7) * 4;

    Op acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b].init();

    auto fetch = [&](int k0) {
        SliceRegs r;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            r.x[i] = load_masked(x, q0 + sr + 32 * i, nx, ldx, k0 + sc, d);
            r.y[i] = load_masked(y, r0 + sr + 32 * i, ny, ldy, k0 + sc, d);
        }
        return r;
    };
    auto stage = [&](const SliceRegs& r) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            *(float4*)(Xs + (sr + 32 * i) * MT_P + sc) = r.x[i];
            *(float4*)(Ys + (sr + 32 * i) * MT_P + sc) = r.y[i];
        }
    };
    const float* xs = Xs + 4 * ty * MT_P;
    const float* ys = Ys + tx * MT_P;
    // four dims at slice offset k into lanes J0 .. J0 + 3 (or the chain, in order)
    auto step4 = [&](int k, auto j0) {
        constexpr int J0 = decltype(j0)::value;
        float4 xv[4], yv[4];
#pragma unroll
        for (int a = 0; a < 4; a++) xv[a] = *(const float4*)(xs + a * MT_P + k);
#pragma unroll
        for (int b = 0; b < 4; b++) yv[b] = *(const float4*)(ys + 16 * b * MT_P + k);
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                acc[a][b].template add<J0>(xv[a].x, yv[b].x, arg);
                acc[a][b].template add<J0 + 1>(xv[a].y, yv[b].y, arg);
                acc[a][b].template add<J0 + 2>(xv[a].z, yv[b].z, arg);
                acc[a][b].template add<J0 + 3>(xv[a].w, yv[b].w, arg);
            }
    };
    // one dim into the chain (LANES == 1)
    auto step1 = [&](int k) {
        float xv[4], yv[4];
#pragma unroll
        for (int a = 0; a < 4; a++) xv[a] = xs[a * MT_P + k];
#pragma unroll
        for (int b = 0; b < 4; b++) yv[b] = ys[16 * b * MT_P + k];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) acc[a][b].template add<0>(xv[a], yv[b], arg);
    };
    using I0 = std::integral_constant<int, 0>;
    using I4 = std::integral_constant<int, 4>;

    const int n8 = d & ~7;
    const int nslice = (d + MT_DS - 1) / MT_DS;
    SliceRegs nxt = fetch(0);
    for (int sl = 0; sl < nslice; sl++) {
        const int k0 = sl * MT_DS;
        __syncthreads();  // the previous slice has been read
        stage(nxt);
        __syncthreads();
        if (sl + 1 < nslice) nxt = fetch(k0 + MT_DS);
        // the slice's share of the 8-dim groups below n8
        const int kb = min(MT_DS, n8 - k0);  // <= 0: none (multiple of 8)
        if (Op::LIBM) {
#pragma unroll 1
            for (int k = 0; k < kb; k++) step1(k);
        } else {
#pragma unroll 2
            for (int k = 0; k < kb; k += 8) {
                step4(k, I0{});
                step4(k + 4, I4{});
            }
        }
    }
    // the dims n8 .. d - 1 lie in the last slice (n8 is 8-aligned, the slices 32-aligned)
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b].fold();
    if (n8 < d) {
        int k = n8 - (nslice - 1) * MT_DS;
        if (Op::LANES == 8) {
            if (d - n8 >= 4) {
                step4(k, I0{});
                k += 4;
            }
            if (d & 3) step4(k, I0{});  // masked_read: zeros beyond d
        } else if (Op::LIBM) {
#pragma unroll 1
            for (; k < d - (nslice - 1) * MT_DS; k++) step1(k);
        } else {
            if (d - n8 >= 4) {
                step4(k, I0{});
                k += 4;
            }
            const int rem = d & 3;
            if (rem > 0) step1(k);
            if (rem > 1) step1(k + 1);
            if (rem > 2) step1(k + 2);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int64_t row = q0 + 4 * ty + a;
        if (row >= nx) continue;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int64_t col = r0 + tx + 16 * b;
            if (col < ny) D[row * ldD + col] = acc[a][b].finish(d);
        }
    }
}

}  // namespace

void metric_distances(const float* x, int64_t nx, int ldx, const float* y, int64_t ny, int ldy,
                      int d, int metric, float metric_arg, float* D, int64_t ldD,
                      hipStream_t s) {
#define METRIC_CASE(MT)                                                                       \
    case MT:                                                                                  \
        if (launch)                                                                           \
            k_metric_tile<MT><<<grid, dim3(256), 0, s>>>(x, nx, ldx, y, ny, ldy, d,           \
                                                         metric_arg, D, ldD, (int)ty);        \
        break
    const bool launch = nx > 0 && ny > 0;
    int64_t tx = 1, ty = 1;
    dim3 grid(1);
    if (launch) {
        FAISS_THROW_IF_NOT(ldx % 4 == 0 && ldy % 4 == 0 && d >= 1 && d <= ldx && d <= ldy);
        tx = (int64_t)cdiv((size_t)nx, MT_Q);
        ty = (int64_t)cdiv((size_t)ny, MT_R);
        FAISS_THROW_IF_NOT(tx * ty < (1ll << 31));
        grid = kgrid(tx * ty, 256);
    }
    switch (metric) {
        METRIC_CASE(M_L1);
        METRIC_CASE(M_Linf);
        METRIC_CASE(M_Lp);
        METRIC_CASE(M_Canberra);
        METRIC_CASE(M_BrayCurtis);
        METRIC_CASE(M_JensenShannon);
        METRIC_CASE(M_Jaccard);
        METRIC_CASE(M_NaNEuclidean);
        METRIC_CASE(M_AbsIP);
        default:
            FAISS_THROW_FMT("Invalid metric %d", metric);  // extra_distances-inl.h:198
    }
#undef METRIC_CASE
    HIP_LAUNCH_CHECK();
}

}  // namespace kern
}  // namespace faiss_amd
