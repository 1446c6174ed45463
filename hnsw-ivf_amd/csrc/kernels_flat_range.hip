// kernels_flat_range.hip — IndexFlat range search (reference
// faiss/IndexFlat.cpp:71-90 -> faiss/utils/distances.cpp:940-966
// range_search_L2sqr / range_search_inner_product with
// RangeSearchBlockResultHandler, faiss/impl/ResultHandler.h:484-608).
//
// Two forms, as the reference picks them (distances.cpp:790-823):
//   * BLAS form (no selector, >= 20 queries): k_pairwise's fp32-MFMA tile
//     (kernels_flat.hip), thresholded while it is in registers.  The tile of
//     distances never reaches HBM.
//   * direct form (a selector, or < 20 queries): ref_dist per pair, one wave
//     per (query, block of rows), the shape of k_ivf_range (kernels_range.hip).
// Both run twice: pass 1 counts the hits of each (query, block of rows), the
// host turns the counts into 64-bit offsets (block order within a query =
// ascending rows = the reference's result order), pass 2 re-evaluates and
// writes each hit at offset + rank, rank = the hits of the same query at
// lower rows of the block.  Distances are recomputed rather than stored, so
// the scratch is 4 B (pass 1) + 8 B (pass 2) per (query, block).
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "flat_tile.h"
#include "kernels.h"
#include "ref_arith.h"

namespace faiss_amd {
namespace kern {

namespace {

static_assert(GB == kFlatRangeTile, "counts are indexed by the contraction tile's columns");

template <bool L2>
__device__ __forceinline__ bool range_admits(float dis, float radius) {
    // C::cmp(radius, dis), strict; false for a NaN on either side
    return L2 ? (dis < radius) : (radius < dis);
}

// One work group per 128 x 128 tile (tile0 + blockIdx.x; consecutive tiles
// walk the row blocks of one 128-query block).  One tile per group and not a
// block-strided loop: inside such a loop this body compiles to 200+ VGPRs
// (one wave per SIMD); this form keeps k_pairwise's budget and its 3 waves
// per SIMD.
template <bool L2, bool FILL>
__global__ __launch_bounds__(256) void k_flat_range_tile(
        const float* __restrict__ x, int64_t nx, int ldx, const float* __restrict__ xn,
        const float* __restrict__ y, int64_t ny, int ldy, const float* __restrict__ yn, int dp,
        float radius, int64_t tiles_y, int64_t tile0, uint32_t* __restrict__ counts,
        const uint64_t* __restrict__ offsets, float* __restrict__ outD,
        int64_t* __restrict__ outI) {
    __shared__ float As[GB * GS];
    __shared__ float Bs[GB * GS];
    // hit bits of the tile: word g of query row r = columns [32 g, 32 g + 32)
    __shared__ uint32_t bits[GB * 4];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int w = t >> 6;
    const int wr = w >> 1, wc = w & 1;
    const int col_l = lane & 31;
    const int rowh = 4 * (lane >> 5);

    const int64_t tile = tile0 + blockIdx.x;
    const int64_t bx = tile / tiles_y;
    const int64_t by = tile - bx * tiles_y;
    const int64_t r0 = bx * GB, c0 = by * GB;

    floatx16 acc[2][2];
    flat_tile_contract(x, nx, ldx, y, ny, ldy, dp, r0, c0, As, Bs, acc);

    // epilogue, in registers.  One accumulator register of one half-wave = 32
    // consecutive columns of one query row, so the two halves of a ballot are
    // the words (row, g) and (row + 4, g).  Every word of the tile is written
    // exactly once (out-of-range pairs as 0).  For the fill the accumulator
    // keeps the distance, or for a pair out of range a value no radius admits.
    const float never = L2 ? INFINITY : -INFINITY;
#pragma unroll
    for (int m = 0; m < 2; m++) {
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const int64_t col = c0 + wc * 64 + n * 32 + col_l;
            const bool colv = col < ny;
            const float ynj = (L2 && colv) ? yn[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row_l = wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + rowh;
                const int64_t row = r0 + row_l;
                float v = never;
                if (colv && row < nx) {
                    const float ip = acc[m][n][r];
                    if (L2) {
                        v = fmaf(-2.f, ip, xn[row] + ynj);
                        if (v < 0.f) v = 0.f;
                    } else {
                        v = ip;
                    }
                }
                const uint64_t b64 = __ballot(range_admits<L2>(v, radius));
                if (col_l == 0)
                    bits[row_l * 4 + wc * 2 + n] = (uint32_t)(lane < 32 ? b64 : (b64 >> 32));
                if (FILL) {
                    // kept opaque and in the accumulator file: otherwise the
                    // second sweep's compares fold into these and 64 ballots
                    // and 64 distances stay live across the barrier
                    float keep = v;
                    asm volatile("" : "+a"(keep));
                    acc[m][n][r] = keep;
                }
            }
        }
    }
    __syncthreads();
    // one thread per query row: the hits of its 128 columns
    if (!FILL) {
        if (t < GB && r0 + t < nx) {
            const uint32_t* bw = bits + t * 4;
            counts[(r0 + t) * tiles_y + by] =
                    __popc(bw[0]) + __popc(bw[1]) + __popc(bw[2]) + __popc(bw[3]);
        }
        return;
    }
    // fill: the row's thread puts where each of its 4 words starts in the
    // output (the cell's offset + the hits at lower words) into LDS, so the
    // sweep below addresses it with immediates and holds no per-row pointers
    __shared__ uint64_t wbase[GB * 4];
    if (t < GB && r0 + t < nx) {
        const uint32_t* bw = bits + t * 4;
        const uint64_t o = offsets[(r0 + t) * tiles_y + by];
        const uint32_t p1 = __popc(bw[0]);
        const uint32_t p2 = p1 + __popc(bw[1]);
        const uint32_t p3 = p2 + __popc(bw[2]);
        uint64_t* wb = wbase + t * 4;
        wb[0] = o; wb[1] = o + p1; wb[2] = o + p2; wb[3] = o + p3;
    }
    __syncthreads();
    // second sweep over the kept distances: the same comparison gives the
    // same ballot; a hit goes to its word's start + the hits at lower lanes
    // of the word (a hit implies row < nx and col < ny).
    const uint32_t below = (1u << col_l) - 1u;
    const uint64_t* wb = wbase + (wr * 64 + rowh) * 4 + wc * 2;
#pragma unroll
    for (int m = 0; m < 2; m++) {
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const int64_t col = c0 + wc * 64 + n * 32 + col_l;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float v = acc[m][n][r];
                const bool hit = range_admits<L2>(v, radius);
                const uint64_t b64 = __ballot(hit);
                if (hit) {
                    const uint32_t mine = (uint32_t)(lane < 32 ? b64 : (b64 >> 32));
                    const uint64_t o =
                            wb[(m * 32 + (r & 3) + 8 * (r >> 2)) * 4 + n] + __popc(mine & below);
                    outD[o] = v;
                    outI[o] = col;
                }
            }
        }
    }
}

// Direct form: one wave per (query, block of kFlatRangeRows rows), lanes take
// 64 consecutive rows, ballot-prefix fill in row order.
template <bool L2, bool FILL>
__global__ __launch_bounds__(64) void k_flat_range_direct(
        const float* __restrict__ x, int ldx, const float* __restrict__ y, int64_t ny, int ldy,
        int d, float radius, const uint8_t* __restrict__ selm, int64_t nblk, int64_t nitems,
        uint32_t* __restrict__ counts, const uint64_t* __restrict__ offsets,
        float* __restrict__ outD, int64_t* __restrict__ outI) {
    const int lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t it = blockIdx.x; it < nitems; it += gridDim.x) {
        const int64_t q = it / nblk;
        const int64_t b = it - q * nblk;
        const float* xq = x + q * (int64_t)ldx;
        const int64_t j0 = b * kFlatRangeRows;
        const int64_t j1 = j0 + kFlatRangeRows < ny ? j0 + kFlatRangeRows : ny;
        const uint64_t base = FILL ? offsets[it] : 0;
        uint32_t cnt = 0;
        for (int64_t jb = j0; jb < j1; jb += 64) {
            const int64_t j = jb + lane;
            bool hit = false;
            float dis = 0.f;
            if (j < j1 && (!selm || selm[j])) {
                dis = ref_dist<L2>(xq, y + j * (int64_t)ldy, d);
                hit = range_admits<L2>(dis, radius);
            }
            const uint64_t m = __ballot(hit);
            if (FILL && hit) {
                const uint64_t o = base + cnt + (uint32_t)__popcll(m & below);
                outD[o] = dis;
                outI[o] = j;
            }
            cnt += (uint32_t)__popcll(m);
        }
        if (!FILL && lane == 0) counts[it] = cnt;
    }
}

// bounded grid, the direct kernel loops over its work items (common.h kgrid)
constexpr int64_t kRangeGridMax = 65536;
// tiles of one k_flat_range_tile launch: 2^30 work-items, inside kgrid's limit
constexpr int64_t kRangeTilesPerLaunch = 1ll << 22;

}  // namespace

void flat_range_tile(const float* x, int64_t nx, int ldx, const float* xn, const float* y,
                     int64_t ny, int ldy, const float* yn, int dp, int metric_l2, float radius,
                     uint32_t* counts, const uint64_t* offsets, float* outD, int64_t* outI,
                     hipStream_t s) {
    if (nx <= 0 || ny <= 0) return;
    FAISS_THROW_IF_NOT(ldx % 4 == 0 && ldy % 4 == 0 && dp % 4 == 0 && dp <= ldx && dp <= ldy);
    FAISS_THROW_IF_NOT(!metric_l2 || (xn && yn));
    const int64_t tx = (int64_t)cdiv(nx, GB), ty = (int64_t)cdiv(ny, GB);
    const int64_t ntiles = tx * ty;
    const bool fill = offsets != nullptr;
    FAISS_THROW_IF_NOT(fill ? (outD && outI) : counts != nullptr);
#define FLAT_RANGE_LAUNCH(L2, F)                                                                 \
    hipLaunchKernelGGL((k_flat_range_tile<L2, F>), grid, dim3(256), 0, s, x, nx, ldx, xn, y, ny, \
                       ldy, yn, dp, radius, ty, tile0, counts, offsets, outD, outI)
    for (int64_t tile0 = 0; tile0 < ntiles; tile0 += kRangeTilesPerLaunch) {
        const dim3 grid = kgrid(std::min(kRangeTilesPerLaunch, ntiles - tile0), 256);
        if (metric_l2) {
            if (fill) FLAT_RANGE_LAUNCH(true, true); else FLAT_RANGE_LAUNCH(true, false);
        } else {
            if (fill) FLAT_RANGE_LAUNCH(false, true); else FLAT_RANGE_LAUNCH(false, false);
        }
        HIP_LAUNCH_CHECK();
    }
#undef FLAT_RANGE_LAUNCH
}

void flat_range_direct(const float* x, int64_t nx, int ldx, const float* y, int64_t ny, int ldy,
                       int d, int metric_l2, float radius, const uint8_t* selm, uint32_t* counts,
                       const uint64_t* offsets, float* outD, int64_t* outI, hipStream_t s) {
    if (nx <= 0 || ny <= 0) return;
    FAISS_THROW_IF_NOT(ldx % 4 == 0 && ldy % 4 == 0 && d <= ldx && d <= ldy);
    const int64_t nblk = (int64_t)cdiv(ny, kFlatRangeRows);
    const int64_t nitems = nx * nblk;
    const dim3 grid = kgrid(std::min(nitems, kRangeGridMax), 64);
    const bool fill = offsets != nullptr;
    FAISS_THROW_IF_NOT(fill ? (outD && outI) : counts != nullptr);
#define FLAT_RANGE_LAUNCH(L2, F)                                                                \
    hipLaunchKernelGGL((k_flat_range_direct<L2, F>), grid, dim3(64), 0, s, x, ldx, y, ny, ldy, \
                       d, radius, selm, nblk, nitems, counts, offsets, outD, outI)
    if (metric_l2) {
        if (fill) FLAT_RANGE_LAUNCH(true, true); else FLAT_RANGE_LAUNCH(true, false);
    } else {
        if (fill) FLAT_RANGE_LAUNCH(false, true); else FLAT_RANGE_LAUNCH(false, false);
    }
#undef FLAT_RANGE_LAUNCH
    HIP_LAUNCH_CHECK();
}

}  // namespace kern
}  // namespace faiss_amd
