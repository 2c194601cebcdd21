// qt_gwa.h -- what the group-wise affine kernels share.  The element arithmetic of dequantization: quantized_ops::dequantize's block
// kernel (qt_groupwise.hip) and the packed-weight kernels (qt_gwa_gemm.hip, qt_gwa_tall.hip) use one definition, so they cannot drift
// apart.  The geometry of the packed layout (described at the head of qt_gwa_gemm.hip), the unpack of a piece and the argument checks
// of the two packed-weight files.
#pragma once
#include "qt_device.h"

namespace {

template <int IO>
__device__ __forceinline__ float rd_io(float f) {            // the result of one torch op in the tensor's dtype
    if constexpr (IO == kIoBf16) return bf16_round(f);
    else return f;
}

// (q - z) * s as two torch ops in the tensor's dtype (decomposed.py:196): both roundings are kept, zero points are not integers
template <int IO>
__device__ __forceinline__ float gwa_dequant(float q, float z, float s) {
    return rd_io<IO>(rd_io<IO>(q - z) * s);
}

// ---- the packed layout -------------------------------------------------------------------------------------------------------------------
template <int BITS>
struct Geo {
    static constexpr int kJ = BITS == 4 ? 4 : 2;      // k steps (of 32) per super step
    static constexpr int kSK = 32 * kJ;               // k per super step
};

inline long gwa_nss(int K, int bits) { return bits == 4 ? (K + 127) / 128 : (K + 63) / 64; }
inline long gwa_pieces(int N, int K, int bits) { return (long)((N + 15) / 16) * gwa_nss(K, bits) * 64; }

// the eight codes of k step j of a lane's 16 bytes, as floats q = code + quant_min (exact)
template <int BITS>
__device__ __forceinline__ void piece_codes(const u32x4 &p, int j, float qmin, float (&q)[8]) {
    const uint32_t w[4] = {p.x, p.y, p.z, p.w};
    if constexpr (BITS == 4) {
        const uint32_t v = w[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = (float)((v >> (4 * e)) & 15u) + qmin;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = (float)((w[2 * j + (e >> 2)] >> (8 * (e & 3))) & 255u) + qmin;
    }
}

// ---- host: argument checks -----------------------------------------------------------------------------------------------------------------
inline bool gwa_aligned(const void *p, uintptr_t n) { return (((uintptr_t)p) & (n - 1)) == 0; }

// log2 of a supported block size, or -1
inline int bs_shift_of(int bs) {
    switch (bs) {
        case 32: return 5;
        case 64: return 6;
        case 128: return 7;
        case 256: return 8;
        case 512: return 9;
        default: return -1;
    }
}

// what every entry point asks of the weight's shape
inline int gwa_shape_status(int N, int K, int bits) {
    if ((bits != 4 && bits != 8) || N < 1 || K < 1) return QT_ERR_BAD_ARG;
    if (K % 32 != 0 || N % 8 != 0) return QT_ERR_UNALIGNED;
    if ((long)N * K > (1L << 40)) return QT_ERR_BAD_ARG;
    return QT_OK;
}

// what the two Linears ask of their arguments.  knobs_ok: the entry point's own tile and split arguments are among the values it takes
// (their place in the precedence: behind the block size, in front of K % block_size).  shift: log2 block_size.
inline int linear_gwa_status(const uint16_t *x, const uint8_t *packed, const uint16_t *scale, const uint16_t *zp, const uint16_t *bias,
                             const uint16_t *y, int M, int N, int K, int block_size, int bits, bool knobs_ok, int &shift) {
    if (!x || !packed || !scale || !zp || !y || M < 0) return QT_ERR_BAD_ARG;
    if (const int rc = gwa_shape_status(N, K, bits)) return rc;
    shift = bs_shift_of(block_size);
    if (shift < 0 || !knobs_ok) return QT_ERR_BAD_ARG;
    if (K % block_size != 0) return QT_ERR_UNALIGNED;
    if ((long)M * K > (1L << 40) || (long)M * N > (1L << 40)) return QT_ERR_BAD_ARG;
    if (!gwa_aligned(x, 16) || !gwa_aligned(packed, 16) || !gwa_aligned(y, 16) || !gwa_aligned(scale, 2) || !gwa_aligned(zp, 2) || !gwa_aligned(bias, 8))
        return QT_ERR_UNALIGNED;
    return QT_OK;
}

}  // namespace
