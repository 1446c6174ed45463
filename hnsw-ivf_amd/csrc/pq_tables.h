// pq_tables.h — the IVF-PQ (query, probe) distance table in the reference's
// arithmetic (QueryTables, faiss/IndexIVFPQ.cpp:545-700), stated once for the
// general exact scan (kernels_exact.hip) and the LDS-table list scan
// (kernels_pq_lut.hip).  Entry arithmetic: pq_ref.h.
//
//   * inner product, or not by residual: the table of x itself,
//     <x_m, c> / |x_m - c|^2; dis0 = <x, y_C> (IP by residual), else 0;
//   * table 1 (L2 by residual, use_precomputed_table == 1):
//     fma(-2, <x_m, c>, P), P = fma(2, <y_C,m, c>, |c|^2) — P depends on the
//     list alone; dis0 = the coarse distance;
//   * table 0 (L2 by residual): |r_m - c|^2 of r = x - y_C; dis0 = 0.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pq_ref.h"
#include "ref_arith.h"

namespace faiss_amd {
namespace kern {

// the list's part of a table-1 entry
__device__ __forceinline__ float pq_list_term(const float* __restrict__ yc_m,
                                              const float* __restrict__ c, int dsub) {
    return fmaf(2.f, ny_entry<false>(yc_m, c, dsub), ref_dist_s<false>(c, c, dsub));
}

// a table-1 entry from the list's part P
__device__ __forceinline__ float pq_table1_entry(const float* xs_m, const float* __restrict__ c,
                                                 int dsub, float P) {
    return fmaf(-2.f, ny_entry<false>(xs_m, c, dsub), P);
}

// one table entry of sub-quantizer m: xs_m / rs_m the query's / residual's
// sub-vector, yc_m the list centroid's, c the sub-centroid
template <bool L2>
__device__ __forceinline__ float pq_table_entry(const ExactPQ& pq, const float* xs_m,
                                                const float* rs_m,
                                                const float* __restrict__ yc_m,
                                                const float* __restrict__ c, int dsub) {
    if (!L2 || !pq.by_residual) {
        // IP table of x (init_query_IP) / distance table of x (not by residual)
        return ny_entry<L2>(xs_m, c, dsub);
    } else if (pq.table1) {
        return pq_table1_entry(xs_m, c, dsub, pq_list_term(yc_m, c, dsub));
    } else {
        return ny_entry<true>(rs_m, c, dsub);
    }
}

// dis0 of a (query, probe): xs the query (d floats), yc the list centroid, cd
// the coarse distance
template <bool L2>
__device__ __forceinline__ float pq_table_dis0(const ExactPQ& pq, const float* xs,
                                               const float* __restrict__ yc, int d, float cd) {
    if (!pq.by_residual) return 0.f;
    if (!L2)  // precompute_list_tables_IP: <x, y_C> (faiss/IndexIVFPQ.cpp:612-628)
        return ref_dist_s<false>(xs, yc, d);
    return pq.table1 ? cd : 0.f;
}

// NB = 8: byte codes, ksub 256 (compile-time); NB = 0: pq.nbits in 4..7,
// packed codes (pq_ref.h pq_index) and the sequential code sum.
template <int NB>
__device__ __forceinline__ int ex_pq_nbits(const ExactPQ& pq) {
    return NB == 8 ? 8 : pq.nbits;
}

// The (query, probe) table in LDS: lut [M * ksub] | xs [ldx] | rs [ldx] | dis0.
// NT threads (the whole work group); returns dis0 (all threads, after the
// barrier).
template <bool L2, int NB, int NT = 256>
__device__ __forceinline__ float ex_pq_tables(const float* __restrict__ xq, int ldx, int d,
                                              int32_t key, float cd, const ExactPQ& pq,
                                              float* lut) {
    const int M = pq.M, dsub = pq.dsub;
    const int nbits = ex_pq_nbits<NB>(pq), ksub = 1 << nbits;
    float* xs = lut + M * ksub;
    float* rs = xs + ldx;
    float* sd0 = rs + ldx;
    const int tid = threadIdx.x;
    const float* yc = pq.cent + (int64_t)key * pq.ldcent;
    for (int i = tid; i < ldx; i += NT) {
        const float v = xq[i];
        xs[i] = v;
        rs[i] = i < d ? v - yc[i] : 0.f;  // Index::compute_residual (faiss/Index.cpp:107-112)
    }
    __syncthreads();
    if (tid == 0) *sd0 = pq_table_dis0<L2>(pq, xs, yc, d, cd);
    for (int ent = tid; ent < M * ksub; ent += NT) {
        const int m = ent >> nbits;
        lut[ent] = pq_table_entry<L2>(pq, xs + m * dsub, rs + m * dsub, yc + m * dsub,
                                      pq.pq_cent + (int64_t)ent * dsub, dsub);
    }
    __syncthreads();
    return *sd0;
}

// floats of LDS ex_pq_tables needs
inline size_t ex_pq_table_floats(int M, int nbits, int ldx) {
    return ((size_t)M << nbits) + 2 * (size_t)ldx + 1;
}

// a row's distance less dis0: the code sum over the table
template <int NB>
__device__ __forceinline__ float ex_pq_code(const float* lut, const ExactPQ& pq,
                                            const uint8_t* code) {
    if constexpr (NB == 8) {
        return pq_code_sum(pq.M, [&](int m) { return lut[m * 256 + code[m]]; });
    } else {
        const int nbits = pq.nbits;
        return pq_code_sum_seq(
                pq.M, [&](int m) { return lut[(m << nbits) + pq_index(code, m, nbits)]; });
    }
}

}  // namespace kern
}  // namespace faiss_amd
