// sq_ref.h — the reference's fp32 evaluation order for scalar-quantizer codes.
//
// faiss/impl/ScalarQuantizer.cpp under the AVX2 flags (faiss/CMakeLists.txt:251)
// with d % 8 == 0, where select_InvertedListScanner takes the 8-wide
// DCTemplate (:1930-2020).  Every step below is one rounded fp32 operation of
// that path, written with explicit fmaf so nothing is left to contraction:
//   * decode (Codec8bit::decode_8_components, :103-114):
//       xi = fma((float)code, 1/255, 0.5/255)
//   * reconstruct (QuantizerTemplate<.., NON_UNIFORM, 8>, :546-553):
//       x^ = fma(xi, vdiff[j], vmin[j]);  vmin = trained[0..d), vdiff = trained[d..2d)
//   * fp16 (QuantizerFP16<8>, :637-641): x^ = the half widened (exact)
//   * L2 (SimilarityL2<8>, :1215-1249): lane j & 7 takes component j,
//       t = y - x^ rounded, acc = fma(t, t, acc)
//   * IP (SimilarityIP<8>, :1375-1412): acc = fma(y, x^, acc)
//   * result_8 of both: s_i = acc[i] + acc[i + 4], then (s0 + s2) + (s1 + s3)
//   * encode (QuantizerTemplate<.., NON_UNIFORM, 1>::encode_vector, :484-498,
//     Codec8bit::encode_component :80-85): xi = (x - vmin) / vdiff clamped to
//     [0, 1] (0 when vdiff == 0), code = (int)(255 * xi); fp16 rounds to
//     nearest even (encode_fp16).
// The d % 8 != 0 path of the reference (DCTemplate<.., 1>) is plain C++ whose
// contraction is the host compiler's choice; it is not restated and such
// indexes are rejected.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace faiss_amd {
namespace kern {

// ScalarQuantizer::QuantizerType values (faiss/impl/ScalarQuantizer.h:27-38)
constexpr int SQ_QT_8bit = 0;
constexpr int SQ_QT_fp16 = 4;

#define SQ_HD __host__ __device__ __forceinline__

SQ_HD float sq_decode8(uint8_t c) { return fmaf((float)c, 1.f / 255.f, 0.5f / 255.f); }
SQ_HD float sq_recons8(uint8_t c, float vmin, float vdiff) {
    return fmaf(sq_decode8(c), vdiff, vmin);
}
// ScalarQuantizer::decode (QuantizerTemplate<.., NON_UNIFORM, 1>::decode_vector,
// :500-505, Codec8bit::decode_component :87-89) is not the scanner's form: the
// component is a true division, xi = (code + 0.5f) / 255.0f, and the
// reference's compiler contracts vmin + xi * vdiff into one fma.  Settled by
// the reference's output for all 256 codes (tests/golden/ref_mutation.npz
// sq_decode: 1144 of 2048 values differ from sq_recons8).
SQ_HD float sq_decode_vector8(uint8_t c, float vmin, float vdiff) {
#ifdef __HIP_DEVICE_COMPILE__
    const float xi = __fdiv_rn((float)c + 0.5f, 255.0f);
#else
    const float xi = ((float)c + 0.5f) / 255.0f;
#endif
    return fmaf(xi, vdiff, vmin);
}
SQ_HD float sq_half_to_float(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
SQ_HD uint16_t sq_float_to_half(float x) {  // round to nearest even
    return __builtin_bit_cast(uint16_t, (_Float16)x);
}

template <bool L2>
SQ_HD float sq_acc(float y, float xr, float acc) {
    if (L2) {
        const float t = y - xr;
        return fmaf(t, t, acc);
    }
    return fmaf(y, xr, acc);
}
// result_8 of SimilarityL2<8> / SimilarityIP<8>
SQ_HD float sq_reduce8(const float* a) {
    const float s0 = a[0] + a[4], s1 = a[1] + a[5], s2 = a[2] + a[6], s3 = a[3] + a[7];
    return (s0 + s2) + (s1 + s3);
}

SQ_HD uint8_t sq_encode8(float x, float vmin, float vdiff) {
    float xi = 0.f;
    if (vdiff != 0.f) {
        xi = (x - vmin) / vdiff;
        if (xi < 0.f) xi = 0.f;
        if (xi > 1.f) xi = 1.f;
    }
    return (uint8_t)(int)(255.f * xi);
}

// distance of y[0..d) to one code row (d % 8 == 0); the form the host uses
// (reconstruction checks) and the model of k_ex_sq's per-row loop
template <bool L2, int QT>
SQ_HD float sq_ref_distance(const float* y, const float* vmin, const float* vdiff,
                            const uint8_t* code, int d) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < d; j++) {
        const float xr = QT == SQ_QT_fp16
                ? sq_half_to_float((uint16_t)(code[2 * j] | ((uint16_t)code[2 * j + 1] << 8)))
                : sq_recons8(code[j], vmin[j], vdiff[j]);
        acc[j & 7] = sq_acc<L2>(y[j], xr, acc[j & 7]);
    }
    return sq_reduce8(acc);
}

#undef SQ_HD

}  // namespace kern
}  // namespace faiss_amd
