// qt_attention_fp8_core.h -- what the attention kernels on FP8 codes share: attention_fp8_split_kernel (qt_attention_fp8.hip, the
// score strip in registers, up to 1024 keys), attention_fp8_long_kernel (qt_attention_fp8_long.hip, the keys streamed, up to 16384) and
// attention_fp8_d32_kernel (qt_attention_fp8_d32.hip, head_dim 32, up to 512 keys; its K image in LDS is its own) and
// attention_fp8_ragged_kernel (qt_attention_fp8_ragged.hip, any key count up to 512).  All hold a wave's 16 query rows against the keys 16 t + 4 g + {0..3} of each 16-key tile t in lane (r, g), read K / V^T blocks that
// arrived by LDS-DMA with the same swizzle, and send the scores through the same rounding chain.
#pragma once
#include "qt_device.h"
#include "qt_attention_split.h"
#include "qt_formats.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int kUnit = 127;                                                        // E8M0 2^0

struct AttnArgs {
    const uint8_t *q8, *k8, *vt8;       // [B][H][Sq][128], [B][H][Sk][128], [B][H][128][Sk] (keys permuted inside 128-blocks)
    const uint16_t *mask;               // additive bf16 or NULL; element strides for (b, h, q), columns contiguous
    long msb, msh, msq;
    const int *row_live;                // optional: one past the last unmasked column per mask row; row strides for (b, h, q)
    long lsb, lsh, lsq;
    int mask_simple;                    // the caller vouches: every mask row is exactly 0 up to its row_live entry and the bf16 minimum from
                                        // there on (causal, right padding) -- the mask is then not read at all
    uint16_t *out;                      // [B][Sq][H][128] bf16; optional when out8 is given (codes only)
    int H, Sq, Sk;
    float scaling;
    uint8_t *out8;                      // optional: the consumer's (output projection's input) stateless FP8 fake-quantizer applied on the way
    qt_format out_fmt;                  // out: `out` (when given) then holds fq(result), out8 its codes, same layout
    const int *mask_irregular;          // optional, device: 0 = qt_mask_row_live_checked found every row "zeros, then the minimum" (as mask_simple)
};

__device__ __forceinline__ int chunk_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// (LDS-DMA: dma16, qt_device.h; the ordinary loads -- mask, fragments -- keep counted waits, the DMA is waited for explicitly with
// vmcnt(0) + barrier)

typedef short v2s __attribute__((ext_vector_type(2)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
// two packed bf16 pairs of probabilities -> four FP8 codes with the hardware conversion (non-saturating: right for values in [0, 1])
template <bool E5M2>
__device__ __forceinline__ uint32_t prob_codes(uint32_t p0, uint32_t p1) {
    v2s o = __builtin_bit_cast(v2s, p0);
    if constexpr (E5M2) {
        o = __builtin_amdgcn_cvt_scalef32_pk_bf8_bf16(o, __builtin_bit_cast(v2bf, p0), 1.0f, false);
        o = __builtin_amdgcn_cvt_scalef32_pk_bf8_bf16(o, __builtin_bit_cast(v2bf, p1), 1.0f, true);
    } else {
        o = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o, __builtin_bit_cast(v2bf, p0), 1.0f, false);
        o = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o, __builtin_bit_cast(v2bf, p1), 1.0f, true);
    }
    return __builtin_bit_cast(uint32_t, o);
}

// scores of the four tiles t0 .. t0 + 3 of one K block.  MODE 0: no mask arithmetic; 1: row-extent mask applied from my_live
// (tiles from `tiles` on lie beyond every row of the wave); 2: additive mask read from mrow.  head_dim 32: f_lo is the lane's 8 bytes of a
// tile, f_hi unused.  MODE + 4, the tail forms (qt_attention_fp8_ragged.hip: the key count is no multiple of 16): the lane's columns
// j * 16 + e >= sk_left do not exist -- their logit is -inf whatever the product and the mask arithmetic gave, a NaN included, and the mask
// (read 2 bytes at a time: its rows may start at any even address) is not read there; tiles from `tiles` on are skipped in every mode
template <int F, int D, int MODE_>
__device__ __forceinline__ void score_half(const uint8_t *blk, int t0, const v8i &qf, int f_lo, int f_hi, float scaling, float (*ev)[4], float &mx,
                                           const uint16_t *mrow, int key0, int my_live, int tiles, int sk_left = 0) {
    constexpr int MODE = MODE_ & 3;
    constexpr bool TAIL = (MODE_ & 4) != 0;
    // staged by hand -- all fragment reads, then the MFMAs back to back, then the rounding chains -- because the compiler keeps
    // source order and a read -> MFMA -> chain sequence per tile exposes the LDS and MFMA latencies four times over
    uint2 m[4];
    if (MODE == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (TAIL) {
                if (j >= tiles) continue;
                const uint16_t *p = mrow + key0 + j * 16;
                const int left = sk_left - j * 16;
                const uint32_t e0 = left > 0 ? p[0] : 0u, e1 = left > 1 ? p[1] : 0u, e2 = left > 2 ? p[2] : 0u, e3 = left > 3 ? p[3] : 0u;
                m[j] = uint2{e0 | (e1 << 16), e2 | (e3 << 16)};
            } else {
                m[j] = *(const uint2 *)(mrow + key0 + j * 16);
            }
        }
    }
    u32x4 klo[4], khi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if ((MODE == 1 || TAIL) && j >= tiles) continue;
        if constexpr (D == 32) {                                         // head_dim 32: 8 bytes of a key, the depth of the 32-deep instruction
            const uint2 k2 = *(const uint2 *)(blk + (t0 + j) * (16 * D) + f_lo);
            klo[j] = u32x4{k2.x, k2.y, 0u, 0u};
        } else {
            klo[j] = *(const u32x4 *)(blk + (t0 + j) * (16 * D) + f_lo);
            if (D == 128) khi[j] = *(const u32x4 *)(blk + (t0 + j) * (16 * D) + f_hi);
            else khi[j] = u32x4{0u, 0u, 0u, 0u};                         // head_dim 64: the upper half of the 128-deep product is 0 x 0
        }
    }
    v4f s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if ((MODE == 1 || TAIL) && j >= tiles) continue;
        if constexpr (D == 32) {                                         // v_mfma_f32_16x16x32_fp8_fp8 / _bf8_bf8: qf's first two words are the fragment
            const long kf = (long)(((unsigned long)klo[j].y << 32) | klo[j].x), q2 = (long)(((unsigned long)(uint32_t)qf[1] << 32) | (uint32_t)qf[0]);
            if constexpr (F == 1) s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8(kf, q2, v4f{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            else s[j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(kf, q2, v4f{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        } else {
            const v8i kf = {(int)klo[j].x, (int)klo[j].y, (int)klo[j].z, (int)klo[j].w, (int)khi[j].x, (int)khi[j].y, (int)khi[j].z, (int)khi[j].w};
            s[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf, v4f{0.f, 0.f, 0.f, 0.f}, F, F, 0, kUnit, 0, kUnit);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if ((MODE == 1 || TAIL) && j >= tiles) {
            ev[j][0] = ev[j][1] = ev[j][2] = ev[j][3] = -INFINITY;
            continue;
        }
        uint32_t w0 = pack_bf16x2(s[j][0], s[j][1]), w1 = pack_bf16x2(s[j][2], s[j][3]);     // the matmul's bf16 output
        w0 = pack_bf16x2(bf_lo(w0) * scaling, bf_hi(w0) * scaling);
        w1 = pack_bf16x2(bf_lo(w1) * scaling, bf_hi(w1) * scaling);
        if (MODE == 2) {
            w0 = pack_bf16x2(bf_lo(w0) + bf_lo(m[j].x), bf_hi(w0) + bf_hi(m[j].x));
            w1 = pack_bf16x2(bf_lo(w1) + bf_lo(m[j].y), bf_hi(w1) + bf_hi(m[j].y));
        }
        float v[4] = {bf_lo(w0), bf_hi(w0), bf_lo(w1), bf_hi(w1)};
        if (MODE == 1) {
            // x + 0 = x; bf16(x + min) = min for every finite x (NaN stays NaN): the mask's effect without reading it
            const int left = my_live - (key0 + j * 16);                    // columns of this lane's four still inside its row's extent
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (e < left || v[e] != v[e]) ? v[e] : -3.3895313892515355e38f;
        }
        if constexpr (TAIL) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = j * 16 + e < sk_left ? v[e] : -INFINITY;
        }
        ev[j][0] = v[0]; ev[j][1] = v[1]; ev[j][2] = v[2]; ev[j][3] = v[3];
        mx = max3(mx, v[0], v[1]);
        mx = max3(mx, v[2], v[3]);
    }
}

// The finished 64 x D tile in LDS on its way out: bf16 values, then codes, rows padded by 16 bytes (which spreads a wave's accesses over
// the banks), so that every lane stores 16 bytes and a wave's store instruction covers whole 128-byte lines of `out` / `out8`.
template <int D> constexpr int kValRow = 2 * D + 16;
template <int D> constexpr int kCodeRow = D + 16;

}  // namespace
