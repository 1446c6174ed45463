// kernels_refine.hip — IndexRefineFlat's exact re-rank of a base index's
// candidates (faiss/IndexRefine.cpp:274-337).
//
// Step 2 of the reference search, IndexFlat::compute_distance_subset
// (faiss/IndexFlat.cpp:92-108 -> fvec_L2sqr_by_idx / fvec_inner_products_by_idx,
// faiss/utils/distances.cpp:974-1020): every candidate's distance becomes
// fvec_L2sqr / fvec_inner_product(x_i, xb[label]) in the reference's fp32 order
// (ref_arith.h); a label < 0 gets +inf (L2) / -inf (IP).  Here the distance is
// written as the exact select's 32-bit key (wave_select.h ex_key) and a label
// < 0 as EX_SKIP: heap_reorder drops label -1 entries and they arrive last in
// a base row, so for reorder_2_heaps (step 3, k_ex_select with SrcRefine in
// kernels_exact.hip) they never arrive.  A label >= ntotal is treated as -1
// and never dereferenced.
//
// Shape: one 64-lane wave per query, 4 queries per 256-thread group, the query
// row in LDS (max(ld, 8 XM) floats per wave, zero beyond ld: the 4-lane form
// reads 8 XM floats of it whatever d is).  Candidates are taken 64 at a time; for 8 <= d <= 8 XM each row
// is read by four lanes (ref_rows64_4lane: a load instruction covers 16 rows x
// 32 contiguous bytes, the 4 lanes of a row complete its cache lines — the
// one-lane-per-row gather of 512-byte rows is bound by the cache lines it
// touches).  Any other d takes one lane per row (ref_dist).
//
// The same evaluator serves IndexRefine::range_search (:169-206): query i's
// hits are labels[lims[i] .. lims[i + 1]), and the distances are plain floats
// (+-inf for a label outside the storage), not filtered by the radius again.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "common.h"
#include "kernels.h"
#include "ref_arith.h"
#include "wave_select.h"

namespace faiss_amd {
namespace kern {

namespace {

constexpr int RF_WAVES = 4;  // queries per work group

// floats of one wave's query copy in LDS (a multiple of 4: rows stay 16-byte aligned)
__host__ __device__ inline int refine_xstride(int ldx, int xm) {
    return ldx > 8 * xm ? ldx : 8 * xm;
}

// XM > 0: four lanes per row, d in [8, 8 XM]; XM == 0: one lane per row.
// RANGE: candidates of query q at [lims[q], lims[q + 1]), float output;
// else at [q * k_base, (q + 1) * k_base), key output.
template <bool L2, int XM, bool RANGE>
__global__ __launch_bounds__(64 * RF_WAVES) void k_refine(
        const float* __restrict__ x, int ldx, int64_t n, int d,
        const int64_t* __restrict__ labels, int64_t k_base,
        const unsigned long long* __restrict__ lims, const float* __restrict__ xb, int ldb,
        int64_t ntotal, uint32_t* __restrict__ keys_out, float* __restrict__ dis_out) {
    // [RF_WAVES][xstride]: ref_rows64_4lane reads 8 XM floats of the query
    // copy whatever d is, so a wave's copy is at least that long, zero beyond ldx
    extern __shared__ float xs[];
    const int xstride = refine_xstride(ldx, XM);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * RF_WAVES + wave;
    float* xr = xs + wave * xstride;
    if (q < n)
        for (int i = lane; i < xstride; i += 64) xr[i] = i < ldx ? x[q * ldx + i] : 0.f;
    __syncthreads();
    if (q >= n) return;
    const int64_t c0 = RANGE ? (int64_t)lims[q] : q * k_base;
    const int64_t cnt = RANGE ? (int64_t)lims[q + 1] - c0 : k_base;
    for (int64_t j0 = 0; j0 < cnt; j0 += 64) {  // wave-uniform
        const int64_t j = j0 + lane;
        const int64_t lab = j < cnt ? labels[c0 + j] : -1;
        const bool valid = lab >= 0 && lab < ntotal;
        float dis;
        if constexpr (XM > 0) {
            dis = ref_rows64_4lane<L2, XM>(xr, xr, xb, ldb, d, (uint32_t)lab, valid, lane);
        } else {
            dis = valid ? ref_dist<L2>(xr, xb + lab * ldb, d) : 0.f;
        }
        if (j < cnt) {
            if constexpr (RANGE) {
                dis_out[c0 + j] = valid ? dis : (L2 ? __builtin_inff() : -__builtin_inff());
            } else {
                keys_out[c0 + j] = valid ? ex_key(dis, L2) : EX_SKIP;
            }
        }
    }
}

template <bool RANGE>
void refine_launch(const float* x, int ldx, int64_t n, int d, int l2, const int64_t* labels,
                   int64_t k_base, const unsigned long long* lims, const float* xb, int ldb,
                   int64_t ntotal, uint32_t* keys_out, float* dis_out, hipStream_t s) {
    if (n <= 0) return;
    // the 4-lane form names a row in 32 bits
    FAISS_THROW_IF_NOT_FMT(ntotal < ((int64_t)1 << 32),
                           "refine storage of %lld rows: at most 2^32 - 1 are served",
                           (long long)ntotal);
    FAISS_THROW_IF_NOT(d >= 1 && ldx >= d && ldb >= d && ldx % 4 == 0 && ldb % 4 == 0);
    const int xm = d < 8 || d > 128 ? 0 : d <= 64 ? 8 : 16;
    const size_t lds = sizeof(float) * RF_WAVES * (size_t)refine_xstride(ldx, xm);
    FAISS_THROW_IF_NOT_FMT(lds <= 64 * 1024, "refine: d = %d does not fit the query tile", d);
    const dim3 grid = kgrid((int64_t)cdiv((size_t)n, RF_WAVES), 64 * RF_WAVES);
#define RF(L2, XM)                                                                          \
    k_refine<L2, XM, RANGE><<<grid, dim3(64 * RF_WAVES), lds, s>>>(                         \
            x, ldx, n, d, labels, k_base, lims, xb, ldb, ntotal, keys_out, dis_out)
#define RFX(XM)          \
    do {                 \
        if (l2)          \
            RF(true, XM);  \
        else             \
            RF(false, XM); \
    } while (0)
    if (xm == 8)
        RFX(8);
    else if (xm == 16)
        RFX(16);
    else
        RFX(0);
#undef RFX
#undef RF
    HIP_LAUNCH_CHECK();
}

}  // namespace

void refine_flat_distances(const float* x, int ldx, int64_t n, int d, int l2,
                           const int64_t* labels, int64_t k_base, const float* xb, int ldb,
                           int64_t ntotal, uint32_t* keys_out, hipStream_t s) {
    FAISS_THROW_IF_NOT(k_base >= 1);
    refine_launch<false>(x, ldx, n, d, l2, labels, k_base, nullptr, xb, ldb, ntotal, keys_out,
                         nullptr, s);
}

void refine_range_distances(const float* x, int ldx, int64_t n, int d, int l2,
                            const unsigned long long* lims, const int64_t* labels,
                            const float* xb, int ldb, int64_t ntotal, float* dis_out,
                            hipStream_t s) {
    refine_launch<true>(x, ldx, n, d, l2, labels, 0, lims, xb, ldb, ntotal, nullptr, dis_out, s);
}

}  // namespace kern
}  // namespace faiss_amd
