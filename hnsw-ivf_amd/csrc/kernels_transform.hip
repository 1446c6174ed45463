// kernels_transform.hip — the linear front end of IndexPreTransform on fp32
// MFMA: y[i, o] = b[o] + sum_j A[o, j] x[i, j] (forward) and
// x[i, j] = sum_o A[o, j] (y[i, o] - b[o]) (transposed, the reverse transform
// of an orthonormal A).  fp32 in, fp32 accumulation, fp32 out.
//
// Work split.  A 256-thread workgroup (4 waves) owns a tile of TM batch rows
// by TN outputs and walks the reduction dimension K in panels of KP = 32.
//   wide   (n > 32):  TM = 128, TN = 64: wave w owns rows 32 w .. 32 w + 31
//                     and both 32-output blocks (2 accumulators of 16 VGPRs)
//   narrow (n <= 32): TM = 32, TN = 128: the four waves share the one 32-row
//                     block, wave w owns outputs 32 w .. 32 w + 31.  A batch
//                     below one MFMA row block spends no workgroup on rows
//                     that do not exist and spreads the matrix over 4x the
//                     waves per output
// The matrix slice of a tile ([TN][K]) is read from HBM once per workgroup,
// panel by panel, never per row.
//
// LDS.  Per panel the batch rows lie as xs[TM][S] and the matrix rows as
// as[TN][S], row-major in k, S = KP + 2 = 34 words; the next panel waits in
// registers (loaded before the MFMAs of the current one, stored after them).
// v_mfma_f32_32x32x2_f32 takes one word per lane from each operand: lane
// (li = lane % 32, lh = lane / 32)
// reads xs[32 wm + li][2 t + lh] and as[32 nb + li][2 t + lh].  S = 2 (mod 4)
// puts li on the 32 even banks (34 li mod 64 = 2 (17 li mod 32), 17 odd) and
// lh on the bank beside it: the 64 lanes of an operand read cover the 64
// banks once.  The panel fill writes consecutive k of a row from consecutive
// lanes (transposed: consecutive outputs, 2-way conflicts on the write only).
//
// Evaluation order (the contract; IndexPreTransform's batch independence
// rests on it).  For output o of row i, with K the reduction length:
//     acc = b[o]                      (forward; 0 when there is no bias or
//                                      in the transposed form)
//     for t = 0 .. ceil(K / 2) - 1:   acc = mfma(acc; u[2 t] v[2 t], u[2 t + 1] v[2 t + 1])
// where u / v are the row's and the matrix's entries (the transposed form's
// u[o] = fl(y[i, o] - b[o])), an index past K - 1 contributes the product
// 0 * 0, and mfma is what one v_mfma_f32_32x32x2_f32 adds to one accumulator
// element from its two k slots.  Every MFMA in the file is that instruction,
// on both tile shapes; rows and outputs of an MFMA block do not interact.  So
// the bits of y[i, o] are a function of (K, row i's values, A, b) alone: not
// of n, the row's position, the tile shape, the wave or the launch split.
//
// Tails: rows past n, outputs past N and k past K are zero-filled in LDS and
// masked at the store; no address outside n x ldx, N x K (the matrix) or
// n x ldy is formed for a load or a store.  Columns N .. ldy - 1 of every
// written row are set to zero by the workgroups of the last output tile.
#include "kernels.h"

namespace faiss_amd {
namespace kern {

namespace {
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int LT_KP = 32;         // reduction panel
constexpr int LT_S = LT_KP + 2;   // LDS row stride (words), 2 mod 4

// WM waves over the rows, 4 / WM over the outputs, NB 32-output blocks each.
// TRANS: the matrix element (output j, k) is A[k * lda + j] and b is
// subtracted from the input instead of starting the accumulator.
template <int WM, int NB, bool TRANS>
__global__ __launch_bounds__(256) void k_linear_transform(
        const float* __restrict__ x, int64_t n, int ldx, const float* __restrict__ A, int lda,
        int K, int N, const float* __restrict__ b, float* __restrict__ y, int ldy,
        uint32_t out_tiles) {
    constexpr int WN = 4 / WM;
    constexpr int TM = 32 * WM, TN = 32 * NB * WN;
    __shared__ float xs[TM * LT_S];
    __shared__ float as[TN * LT_S];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    const int64_t row0 = (int64_t)(blockIdx.x / out_tiles) * TM;
    const int o0 = (int)(blockIdx.x % out_tiles) * TN;

    floatx16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
        const int o = o0 + (wn * NB + nb) * 32 + li;
        const float v = (!TRANS && b && o < N) ? b[o] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[nb][r] = v;
    }

    // One panel ahead in registers: the global loads of panel p + 1 are in
    // flight while the MFMAs of panel p run; they reach LDS after the barrier
    // that ends panel p.  (What is loaded, and the order it is accumulated
    // in, are those of the plain loop.)
    constexpr int XE = TM * LT_KP / 256, AE = TN * LT_KP / 256;
    float xv[XE], av[AE];
    auto fetch = [&](int k0) {
        // batch panel: lanes along k (one 128-byte line of a row per half wave)
#pragma unroll
        for (int i = 0; i < XE; i++) {
            const int e = tid + 256 * i;
            const int64_t gr = row0 + e / LT_KP;
            const int gk = k0 + e % LT_KP;
            float v = 0.f;
            if (gr < n && gk < K) {
                v = x[gr * ldx + gk];
                if (TRANS && b) v -= b[gk];
            }
            xv[i] = v;
        }
#pragma unroll
        for (int i = 0; i < AE; i++) {
            const int e = tid + 256 * i;
            // transposed: lanes along the outputs, contiguous in A's rows there
            const int o = TRANS ? e % TN : e / LT_KP, k = TRANS ? e / TN : e % LT_KP;
            const int go = o0 + o, gk = k0 + k;
            av[i] = (go < N && gk < K) ? (TRANS ? A[(int64_t)gk * lda + go] : A[(int64_t)go * lda + gk])
                                       : 0.f;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < XE; i++) {
            const int e = tid + 256 * i;
            xs[(e / LT_KP) * LT_S + e % LT_KP] = xv[i];
        }
#pragma unroll
        for (int i = 0; i < AE; i++) {
            const int e = tid + 256 * i;
            const int o = TRANS ? e % TN : e / LT_KP, k = TRANS ? e / TN : e % LT_KP;
            as[o * LT_S + k] = av[i];
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += LT_KP) {
        stage();
        __syncthreads();
        if (k0 + LT_KP < K) fetch(k0 + LT_KP);
        const int steps = (min(LT_KP, K - k0) + 1) >> 1;  // block-uniform
        const float* xr = xs + (wm * 32 + li) * LT_S + lh;
        const float* ar = as + (wn * NB * 32 + li) * LT_S + lh;
        for (int t = 0; t < steps; t++) {
            const float u = xr[2 * t];
#pragma unroll
            for (int nb = 0; nb < NB; nb++)
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(u, ar[nb * 32 * LT_S + 2 * t],
                                                              acc[nb], 0, 0, 0);
        }
        __syncthreads();
    }

    // accumulator register r of lane (li, lh): row 8 (r / 4) + 4 lh + r % 4 of
    // the wave's block, output li of block nb: a half wave stores 128 bytes
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
        const int o = o0 + (wn * NB + nb) * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int64_t gr = row0 + wm * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
            if (gr < n && o < N) y[gr * ldy + o] = acc[nb][r];
        }
    }
    // pad columns N .. ldy - 1 of this tile's rows (last output tile only)
    if (blockIdx.x % out_tiles == out_tiles - 1) {
        const int pad = ldy - N;
        for (int e = tid; e < TM * pad; e += 256) {
            const int64_t gr = row0 + e / pad;
            if (gr < n) y[gr * ldy + N + e % pad] = 0.f;
        }
    }
}

template <int WM, int NB>
void launch_variant(const float* x, int64_t n, int ldx, const float* A, int lda, int K, int N,
                    const float* b, float* y, int ldy, bool trans, hipStream_t s) {
    constexpr int TM = 32 * WM, TN = 32 * NB * (4 / WM);
    const int64_t out_tiles = (int64_t)cdiv((size_t)N, TN);
    // row tiles per launch: inside kgrid's 2^32 work-item count
    const int64_t max_rt = std::max<int64_t>(1, ((int64_t)1 << 23) / out_tiles);
    const int64_t row_tiles = (int64_t)cdiv((size_t)n, TM);
    for (int64_t t0 = 0; t0 < row_tiles; t0 += max_rt) {
        const int64_t nt = std::min(max_rt, row_tiles - t0);
        const int64_t r0 = t0 * TM;
        const int64_t nr = std::min<int64_t>(n - r0, nt * TM);
        const dim3 grid = kgrid(nt * out_tiles, 256);
        if (trans)
            k_linear_transform<WM, NB, true><<<grid, dim3(256), 0, s>>>(
                    x + r0 * ldx, nr, ldx, A, lda, K, N, b, y + r0 * ldy, ldy, (uint32_t)out_tiles);
        else
            k_linear_transform<WM, NB, false><<<grid, dim3(256), 0, s>>>(
                    x + r0 * ldx, nr, ldx, A, lda, K, N, b, y + r0 * ldy, ldy, (uint32_t)out_tiles);
        HIP_LAUNCH_CHECK();
    }
}

void launch(const float* x, int64_t n, int ldx, const float* A, int d_in, int d_out,
            const float* b, float* y, int ldy, bool trans, int variant, hipStream_t s) {
    FAISS_THROW_IF_NOT_FMT(d_in >= 1 && d_in <= kTransformMaxDim,
                           "linear_transform: d_in = %d is outside 1 .. %d", d_in,
                           kTransformMaxDim);
    FAISS_THROW_IF_NOT_FMT(d_out >= 1 && d_out <= kTransformMaxDim,
                           "linear_transform: d_out = %d is outside 1 .. %d", d_out,
                           kTransformMaxDim);
    const int K = trans ? d_out : d_in, N = trans ? d_in : d_out;
    FAISS_THROW_IF_NOT_FMT(ldx >= K && ldy >= N,
                           "linear_transform: leading dimensions %d / %d below the row lengths "
                           "%d / %d",
                           ldx, ldy, K, N);
    FAISS_THROW_IF_NOT_MSG(x != y, "linear_transform: in-place transform is not served");
    if (n <= 0) return;
    const bool narrow = variant == 0 ? n <= kTransformNarrowRows : variant == 2;
    if (narrow)
        launch_variant<1, 1>(x, n, ldx, A, d_in, K, N, b, y, ldy, trans, s);
    else
        launch_variant<4, 2>(x, n, ldx, A, d_in, K, N, b, y, ldy, trans, s);
}
}  // namespace

void linear_transform(const float* x, int64_t n, int ldx, const float* A, int d_in, int d_out,
                      const float* b, float* y, int ldy, hipStream_t s, int variant) {
    launch(x, n, ldx, A, d_in, d_out, b, y, ldy, false, variant, s);
}

void linear_transform_transposed(const float* y, int64_t n, int ldy, const float* A, int d_in,
                                 int d_out, const float* b, float* x, int ldx, hipStream_t s,
                                 int variant) {
    launch(y, n, ldy, A, d_in, d_out, b, x, ldx, true, variant, s);
}

}  // namespace kern
}  // namespace faiss_amd
