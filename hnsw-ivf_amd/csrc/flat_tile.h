// flat_tile.h — the fp32-MFMA contraction tile of the BLAS form, shared by
// k_pairwise (kernels_flat.hip) and k_flat_range_tile (kernels_flat_range.hip)
// so that the reference-pinned arithmetic exists once.
//
// 256 threads = 4 waves; CTA tile 128 (x rows) x 128 (y rows); each wave
// owns a 64x64 quadrant as 2x2 MFMA 32x32 accumulators.  K staged in chunks of
// 32 dims through LDS with a 33-float row stride (conflict-free column reads).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace faiss_amd {
namespace kern {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int GB = 128;
constexpr int GK = 32;
constexpr int GS = GK + 1;

// acc[m][n] += <x rows, y rows> over k = 0 .. dp-1 in ascending k (one fma per
// k: v_mfma_f32_32x32x2_f32 is an exact f32 fma chain), for the quadrant
// (wr, wc) = (wave >> 1, wave & 1) of the tile at (r0, c0).  As and Bs are
// GB * GS floats of LDS each; rows past nx / ny and dims past dp read as 0.
// Ends on a barrier, so the caller may reuse As / Bs at once.
// C/D map of acc[m][n][r]: col = c0 + wc*64 + n*32 + (lane & 31),
// row = r0 + wr*64 + m*32 + (r & 3) + 8*(r >> 2) + 4*(lane >> 5).
__device__ __forceinline__ void flat_tile_contract(const float* __restrict__ x, int64_t nx,
                                                   int ldx, const float* __restrict__ y,
                                                   int64_t ny, int ldy, int dp, int64_t r0,
                                                   int64_t c0, float* As, float* Bs,
                                                   floatx16 (&acc)[2][2]) {
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int w = t >> 6;
    const int wr = w >> 1, wc = w & 1;
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

    for (int k0 = 0; k0 < dp; k0 += GK) {
#pragma unroll
        for (int s = 0; s < 4; s++) {
            int e = t + 256 * s;
            int r = e >> 3, c4 = e & 7;
            int kc = k0 + 4 * c4;
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (r0 + r < nx && kc < dp) va = *(const float4*)(x + (r0 + r) * ldx + kc);
            if (c0 + r < ny && kc < dp) vb = *(const float4*)(y + (c0 + r) * ldy + kc);
            float* pa = As + r * GS + 4 * c4;
            float* pb = Bs + r * GS + 4 * c4;
            pa[0] = va.x; pa[1] = va.y; pa[2] = va.z; pa[3] = va.w;
            pb[0] = vb.x; pb[1] = vb.y; pb[2] = vb.z; pb[3] = vb.w;
        }
        __syncthreads();
        const int li = lane & 31, lk = lane >> 5;
        const float* a0p = As + (wr * 64 + li) * GS + lk;
        const float* a1p = a0p + 32 * GS;
        const float* b0p = Bs + (wc * 64 + li) * GS + lk;
        const float* b1p = b0p + 32 * GS;
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2) {
            float a0 = a0p[kk], a1 = a1p[kk], b0 = b0p[kk], b1 = b1p[kk];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
}

}  // namespace kern
}  // namespace faiss_amd
