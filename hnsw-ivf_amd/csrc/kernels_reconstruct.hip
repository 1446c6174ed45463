// kernels_reconstruct.hip — gather and decode of result rows for
// IndexIVF::search_and_reconstruct (faiss/IndexIVF.cpp:1495-1511).
//
// One wave per result slot.  The slot's label is the lo_build(list, offset)
// pair a store_pairs search left; the wave turns it into the arena row, copies
// the row's slot of the arena into LDS (16 bytes per lane and load, the few
// bytes a slot has beyond its last whole 16 in 4-byte pieces — a slot is a
// multiple of 4 bytes — so nothing outside the slot is read), and decodes from
// LDS one component per lane with coalesced float stores:
//   Flat    the float itself (faiss/IndexIVFFlat.cpp reconstruct_from_offset)
//   PQ      centroid [m][index m][j % dsub], index m from the packed bit stream
//           (pq_ref.h pq_index: a field may straddle two bytes)
//   SQ8     sq_ref.h sq_decode_vector8 (ScalarQuantizer::decode's arithmetic)
//   SQfp16  the half widened
// and, when by_residual, one rounded add of the list's coarse centroid
// (faiss/IndexIVFPQ.cpp:325-327, faiss/IndexScalarQuantizer.cpp:273-275).
// A negative label stays and its d words become 0xFFFFFFFF (the reference's
// memset(-1)); so does a pair that names no stored row (never produced by the
// scan; checked because the labels are a caller's device memory).
#include "kernels.h"
#include "pq_ref.h"
#include "sq_ref.h"

namespace faiss_amd {
namespace kern {

namespace {

constexpr int RC_WAVES = 4;        // slots per work group
constexpr int RC_CHUNK = 4096;     // bytes of a row staged per pass and wave

typedef uint32_t rc_u4 __attribute__((ext_vector_type(4), aligned(4)));

__global__ __launch_bounds__(64 * RC_WAVES) void k_reconstruct_pairs(
        ReconsArgs a, int64_t n, int64_t* __restrict__ labels, float* __restrict__ recons) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[RC_WAVES][RC_CHUNK];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t slot = (int64_t)blockIdx.x * RC_WAVES + wid;
    // wave-uniform: the slot's row (-1: none)
    int64_t row = -1;
    uint32_t list = 0;
    if (slot < n) {
        const int64_t lo = labels[slot];
        if (lo >= 0) {
            const uint64_t l = (uint64_t)lo >> 32, o = (uint64_t)lo & 0xffffffffull;
            if (l < (uint64_t)a.nlist && o < (uint64_t)a.list_len[l]) {
                list = (uint32_t)l;
                row = (int64_t)a.list_off[l] + (int64_t)o;
            }
        }
    }
    float* out = slot < n ? recons + slot * a.d : nullptr;
    if (slot < n && row < 0) {
        for (int j = lane; j < a.d; j += 64) out[j] = __uint_as_float(0xffffffffu);
        if (lane == 0) labels[slot] = -1;
    }
    if (slot < n && row >= 0 && lane == 0) labels[slot] = a.ids[row];
    const uint8_t* src = row >= 0 ? a.codes + row * (int64_t)a.stride : nullptr;
    const float* cent = (a.by_residual && row >= 0) ? a.cent + (int64_t)list * a.ldcent : nullptr;
    // bytes of a component's code: Flat 4, SQ8 1, SQfp16 2; PQ rows take one pass
    const int bpc = a.kind == RECONS_FLAT ? 4 : a.kind == RECONS_SQFP16 ? 2 : 1;
    uint8_t* st = stage[wid];
    // (the pass count is the same for every wave of the group: barriers inside)
    for (int c0 = 0; c0 < a.stride; c0 += RC_CHUNK) {
        const int cb = min(RC_CHUNK, a.stride - c0);  // multiple of 4
        const int n16 = cb >> 4;
        if (src) {
            for (int p = lane; p < n16; p += 64)
                *(uint4*)(st + 16 * p) =
                        __builtin_bit_cast(uint4, *(const rc_u4*)(src + c0 + 16 * p));
            const int n4 = (cb - 16 * n16) >> 2;
            if (lane < n4)
                *(uint32_t*)(st + 16 * n16 + 4 * lane) =
                        *(const uint32_t*)(src + c0 + 16 * n16 + 4 * lane);
        }
        __syncthreads();
        if (src) {
            if (a.kind == RECONS_PQ) {
                for (int j = lane; j < a.d; j += 64) {
                    const int m = j / a.dsub, w = j - m * a.dsub;
                    const int c = pq_index(st, m, a.nbits);
                    float v = a.pq_cent[((int64_t)m * (1 << a.nbits) + c) * a.dsub + w];
                    if (cent) v = v + cent[j];
                    out[j] = v;
                }
            } else {
                const int j1 = min(a.d, (c0 + cb) / bpc);
                for (int j = c0 / bpc + lane; j < j1; j += 64) {
                    const uint8_t* p = st + (j * bpc - c0);
                    float v;
                    if (a.kind == RECONS_FLAT)
                        v = *(const float*)p;
                    else if (a.kind == RECONS_SQFP16)
                        v = sq_half_to_float(*(const uint16_t*)p);
                    else
                        v = sq_decode_vector8(*p, a.trained[j], a.trained[a.d + j]);
                    if (cent) v = v + cent[j];
                    out[j] = v;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

void ivf_reconstruct_pairs(const ReconsArgs& a, int64_t n, int64_t* labels, float* recons,
                           hipStream_t s) {
    if (n <= 0) return;
    FAISS_THROW_IF_NOT(a.kind >= RECONS_FLAT && a.kind <= RECONS_SQFP16);
    FAISS_THROW_IF_NOT(a.d > 0 && a.stride > 0 && (a.stride & 3) == 0 && a.codes && a.ids);
    const int bpc = a.kind == RECONS_FLAT ? 4 : a.kind == RECONS_SQFP16 ? 2 : 1;
    if (a.kind == RECONS_PQ) {
        FAISS_THROW_IF_NOT(a.M > 0 && a.dsub > 0 && a.M * a.dsub == a.d && a.nbits >= 4 &&
                           a.nbits <= 8 && a.pq_cent);
        FAISS_THROW_IF_NOT_FMT((a.M * a.nbits + 7) / 8 <= a.stride && a.stride <= RC_CHUNK,
                               "PQ code rows of %d bytes are beyond this kernel's %d", a.stride,
                               RC_CHUNK);
    } else {
        FAISS_THROW_IF_NOT((int64_t)a.d * bpc <= a.stride);
        FAISS_THROW_IF_NOT(a.kind != RECONS_SQ8 || a.trained);
    }
    FAISS_THROW_IF_NOT(!a.by_residual || a.cent);
    k_reconstruct_pairs<<<kgrid((int64_t)cdiv((size_t)n, RC_WAVES), 64 * RC_WAVES),
                          dim3(64 * RC_WAVES), 0, s>>>(a, n, labels, recons);
    HIP_LAUNCH_CHECK();
}

}  // namespace kern
}  // namespace faiss_amd
