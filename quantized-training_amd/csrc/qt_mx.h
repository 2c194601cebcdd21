// Element codes of the block-scaled formats the matrix instruction takes (OCP MX v1.0 element formats).
#pragma once
#include <stdint.h>

#include "qt_device.h"
#include "qt_formats.h"
#include "qt_mx_log2_tables.h"

namespace qt_mx {

__host__ __device__ constexpr int elem_bits(int f) { return f < 2 ? 8 : (f < 4 ? 6 : 4); }

// value -> code of format f (QT_MX_*).  A value the format holds exactly converts exactly; anything else sets `bad`.
__device__ __forceinline__ uint32_t encode_elem(int f, float v, bool &bad) {
    const uint32_t u = qt_f2u(v), s = u >> 31, au = u & 0x7FFFFFFFu;
    const float m = qt_u2f(au);
    const int E = (int)(au >> 23) - 127;
    int ebits, mbits, bias;
    float maxv;
    switch (f) {
        case 0: ebits = 4; mbits = 3; bias = 7; maxv = 448.f; break;
        case 1: ebits = 5; mbits = 2; bias = 15; maxv = 57344.f; break;
        case 2: ebits = 2; mbits = 3; bias = 1; maxv = 7.5f; break;
        case 3: ebits = 3; mbits = 2; bias = 3; maxv = 28.f; break;
        default: ebits = 2; mbits = 1; bias = 1; maxv = 6.f; break;
    }
    if (!(m <= maxv)) { bad = true; return 0; }          // also catches NaN
    uint32_t code;
    float back;
    if (E < 1 - bias) {                                  // subnormal of the target: multiples of 2^(1 - bias - mbits)
        const float q = m * qt_u2f((uint32_t)(127 - (1 - bias - mbits)) << 23);
        code = (uint32_t)q;
        back = (float)code * qt_u2f((uint32_t)(127 + (1 - bias - mbits)) << 23);
    } else {
        const uint32_t mant = (au >> (23 - mbits)) & ((1u << mbits) - 1u);
        code = ((uint32_t)(E + bias) << mbits) | mant;
        back = qt_u2f(au & ~((1u << (23 - mbits)) - 1u));
    }
    if (back != m) bad = true;
    (void)ebits;
    return code | (s << (ebits + mbits));
}

// ---- what the quantize_mx kernels (csrc/qt_mx_quant.hip: blocks along the last axis, blocks along any other axis) share ----------------

// floor of log2(a) as the reference computes it in dtype IO (a > 0 finite, given as its fp32 bit image): the exponent,
// plus one when the mantissa is high enough for the dtype-rounded logarithm to reach the next integer
// (thresholds: qt_mx_log2_tables.h, generated from torch's own CPU log2 by tools/gen_mx_log2_tables.py).
template <int IO>
__device__ __forceinline__ int floor_log2_dtype(uint32_t au) {
    const uint32_t E = au >> 23, M = au & 0x7FFFFFu;
    int e;
    uint32_t mn;
    if (E) { e = (int)E - 127; mn = M; }
    else { const int p = 31 - __clz((int)M); e = p - 149; mn = (M << (23 - p)) & 0x7FFFFFu; }
    const uint32_t thr = (IO == kIoBf16 ? kMxLog2ThrBf16 : kMxLog2ThrF32)[e + 1 - kMxLog2Lo];
    return e + (mn >= thr ? 1 : 0);
}

// The scale of one block, and what the element pass and the pack derive from it.
struct BlockScale {
    float s;             // in the tensor's dtype
    int se;              // s = 2^se when is_pow2
    bool is_pow2;        // force_pow2 and 2^se representable
    // x * 2^-se is x / s exactly where both powers are normal numbers
    __device__ __forceinline__ bool recip_ok() const { return is_pow2 && se >= -126 && se <= 126; }
    __device__ __forceinline__ float recip() const { return recip_ok() ? qt_u2f((uint32_t)(127 - se) << 23) : 0.0f; }
    // E8M0 holds 2^-127 .. 2^127: a block whose scale is lower (|x| below ~1e-36) is flushed to zeros,
    // an absolute error under 2^-119 per element; scale 1 from the where() guard is byte 127.
    __device__ __forceinline__ bool flush() const { return is_pow2 && se < -127; }
    __device__ __forceinline__ uint8_t e8m0() const {
        const int eb = is_pow2 ? se + 127 : 127;
        return (uint8_t)(eb < 0 ? 0 : eb);
    }
};

// calculate_mx_qparam for one block (decomposed.py:365-448) from the block's amax as an absolute bit pattern (NaN patterns win the
// integer maximum): 2 ** (floor(log2(amax + 2^-126 (amax == 0))) - qmax_exp) with its NaN / Inf / underflow / overflow cases, or
// amax / quant_max [-> scale map]; then where(s > 0, s, 1).
template <int IO>
__device__ __forceinline__ BlockScale block_scale(uint32_t am, bool pow2, float quant_max, int qmax_exp, const uint16_t *scale_lut) {
    BlockScale b{1.0f, 0, false};
    if (pow2) {
        if (am > 0x7F800000u) b.s = 1.0f;                  // NaN: 2 ** NaN = NaN, where(NaN > 0) -> 1
        else if (am == 0x7F800000u) b.s = qt_u2f(0x7F800000u);   // +Inf stays +Inf
        else {
            b.se = floor_log2_dtype<IO>(am ? am : 0x00800000u) - qmax_exp;   // + FP32_MIN_NORMAL * (amax == 0)
            const int lowest = IO == kIoBf16 ? -133 : -149;                 // smallest power of two of the dtype
            if (b.se < lowest) b.s = 1.0f;                                  // 2 ** e underflows to 0 -> 1
            else if (b.se > 127) b.s = qt_u2f(0x7F800000u);
            else {
                b.s = b.se >= -126 ? qt_u2f((uint32_t)(b.se + 127) << 23) : qt_u2f(1u << (b.se + 149));
                b.is_pow2 = true;
            }
        }
    } else {
        float s = qt_u2f(am) / quant_max;
        if constexpr (IO == kIoBf16) s = qt_u2f(pack_bf16x2(s, 0.0f) << 16);
        if (scale_lut) {
            const uint32_t img = IO == kIoBf16 ? qt_f2u(s) : qt_fold_img(qt_f2u(s));
            s = qt_bf2f(scale_lut[img >> 16]);
        }
        b.s = s > 0.0f ? s : 1.0f;
    }
    return b;
}

// value (exactly representable in the target format) -> element code; mbits / bias / ebits of the target at run time
__device__ __forceinline__ uint32_t encode_exact(float v, int ebits, int mbits, int bias) {
    const uint32_t u = qt_f2u(v), au = u & 0x7FFFFFFFu;
    const int E = (int)(au >> 23) - 127;
    const uint32_t normal = ((uint32_t)(E + bias) << mbits) | ((au >> (23 - mbits)) & ((1u << mbits) - 1u));
    const uint32_t sub = (uint32_t)(qt_u2f(au) * qt_u2f((uint32_t)(127 + bias - 1 + mbits) << 23));     // multiples of 2^(1 - bias - mbits)
    return (E >= 1 - bias ? normal : sub) | ((u >> 31) << (ebits + mbits));
}

// The element codes of one vector of N (8 or 4) on-grid values, BITS wide, packed: 8-bit -- w[0], w[1] hold four bytes each;
// 6-bit -- w[0], w[1] hold four codes in 24 bits each; 4-bit -- w[0] holds all nibbles.  code(i) takes one out again.
template <int BITS>
struct VecCodes {
    uint32_t w[2];
    __device__ __forceinline__ uint32_t code(int i) const {
        if constexpr (BITS == 4) return (w[0] >> (4 * i)) & 15u;
        else return (w[i >> 2] >> (BITS * (i & 3))) & ((1u << BITS) - 1u);
    }
};

template <int BITS, int N>
__device__ __forceinline__ VecCodes<BITS> vec_codes(const float (&qv)[N], int f) {
    static_assert(N == 8 || N == 4, "one 16-byte vector of bf16 or fp32");
    VecCodes<BITS> out{{0u, 0u}};
    // 8- and 4-bit elements: the values are on the format's grid, so the hardware conversions give their codes
    // exactly (v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32, v_cvt_scalef32_pk_fp4_f32 with scale 1) -- half an
    // instruction per element instead of the ~8 of encode_exact, on a kernel that is issue-limited
    if constexpr (BITS == 8 && N == 8) {
        if (f == 0) { out.w[0] = qt_pack_fp8x4<false>(qv[0], qv[1], qv[2], qv[3]); out.w[1] = qt_pack_fp8x4<false>(qv[4], qv[5], qv[6], qv[7]); }
        else { out.w[0] = qt_pack_fp8x4<true>(qv[0], qv[1], qv[2], qv[3]); out.w[1] = qt_pack_fp8x4<true>(qv[4], qv[5], qv[6], qv[7]); }
    } else if constexpr (BITS == 4 && N == 8) {
        uint32_t w4 = 0;
        w4 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w4, qv[0], qv[1], 1.0f, 0);
        w4 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w4, qv[2], qv[3], 1.0f, 1);
        w4 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w4, qv[4], qv[5], 1.0f, 2);
        w4 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w4, qv[6], qv[7], 1.0f, 3);
        out.w[0] = w4;
    } else {
        const int ebits = BITS == 8 ? (f == 0 ? 4 : 5) : (BITS == 6 ? (f == 2 ? 2 : 3) : 2);
        const int mbits = BITS - 1 - ebits;
        const int bias = (1 << (ebits - 1)) - 1;
        uint32_t c[N];
#pragma unroll
        for (int e = 0; e < N; ++e) c[e] = encode_exact(qv[e], ebits, mbits, bias) & ((1u << BITS) - 1u);   // Inf / NaN stay in their own bits
        if constexpr (BITS == 4) {
#pragma unroll
            for (int e = 0; e < N; ++e) out.w[0] |= c[e] << (4 * e);
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) out.w[e >> 2] |= c[e] << (BITS * (e & 3));
        }
    }
    return out;
}

}  // namespace qt_mx
