// qt_attention_mxi.hip -- the attention core of the block-scaled INTEGER recipe in one launch (plus a small prepare launch):
// Q.K^T, scaling, mask, softmax, the block quantizer of the probabilities and P.V, the B x H x S x S tensors never written.
//
// Replaces, in a converted graph whose two attention matmuls run as
//     int6,qs=microscaling,bs=64,ax=-1[,scale=fp8_e5m3]  x  int6,qs=microscaling,bs=64,ax=-2[,scale=fp8_e5m3]
// (examples/language_modeling/prepare_model.py: matmul6, linear4_matmul6_fp8 and their variants), the span
//     matmul_mx(q, k^T)  ->  mul / div by a scalar  ->  + mask  ->  softmax(-1)  ->  quantize_mx(p, ax=-1)  ->  matmul_mx(p', v)
//                                                                    decomposed.py:304-363 (matmul_mx), 365-448 (quantize_mx)
// on the operands qt_mxi_pack writes for those matmuls: int8 codes q [B][H][Q][D], k [B][H][C][D] (the rows view of K^T, blocks along
// D), v [B][H][D][C] (N-major, blocks along the keys) with fp32 scales [..][D/64], [..][D/64], [..][C/64].  bf16 graphs, block size 64.
//
// Rounding chain -- that of the nodes the launch replaces:
//   1. scores   per 64-block of head_dim the exact int32 sum (one v_mfma_i32_16x16x64_i8) times fl32(s_q s_k), fma'd in ascending block
//               order from 0 (mxi_block's order, qt_mxi_gemm's bits), one rounding to bf16;
//   2. scaling  bf16(t * c) or bf16(t / c), c in fp32.  t / c is the correctly rounded fp32 quotient: the CPU node's and the reference's.
//               torch's DEVICE node divides by a Python scalar or a 0-dim CPU constant as t * fl32(1 / c) (upstream's
//               div_true_kernel_cuda, read, not run), which can differ from it by one bf16 step on rare elements next to a bf16 tie;
//               for c a power of two the two are equal;
//   3. mask     bf16(t + mask);
//   4. softmax  in fp32 on those bf16 logits over the whole row, rounded to bf16 once;
//   5. P's quantizer (quantize_mx_kernel, csrc/qt_mx_quant.hip): per (row, 64-key block) amax -> qt_mx::block_scale<kIoBf16> -> the scale
//               as a bf16 value; per element map(bf16(p / s)) -- p * 2^-e where the scale is a power of two with a normal reciprocal --
//               with map = the closed form of intN (round half even, clamp);
//   6. P.V      per 64-key block the exact int32 sum times fl32(s_p s_v), fma'd in ascending key-block order, one rounding to bf16.
// A row whose logits are all -inf is NaN (softmax's 0 / 0); a row whose logits are all the bf16 minimum is the uniform row.
//
// P's block scale needs the NORMALISED probability, so the row maximum and the sum of exponentials are final before any code is formed:
// the keys are streamed twice, as in qt_attention_fp8_long.hip.
//   sweep 1   K blocks of 64 keys (codes and scales) through a ring of three LDS stages; per block the 4 score tiles, the running
//             maximum and the running sum, lane-local; the four partial sums of a row meet in two shuffles behind the last block.
//   sweep 2   K and V^T blocks through the same ring; the same score tiles again (same instruction, same operands: the same bits),
//             p = bf16(exp2((t - m) log2e) / l), the block amax of a row over the four lanes g = 0..3 (two shuffles), the scale, the 16
//             codes of the lane, P.V.
// A workgroup = 4 waves owns 64 query rows of one (b, h), a wave 16 of them, and walks ALL keys: nothing but the ring passes through LDS
// and the only barriers are the ring's.  The operands are multiplied swapped (K fragment first): lane (r, g) holds query r against keys
// 16 t + 4 g + {0..3} of each 16-key tile t, so the four tiles of a 64-block leave 16 probabilities of ONE block in the lane -- byte
// 4 t + i of the 16-byte B fragment of v_mfma_i32_16x16x64_i8 is key 16 t + 4 g + i.  V^T's keys are permuted to match inside each
// 64-block by the PREPARE launch of this file (mxi_attention_prepare_kernel: a 4 x 4 transpose of the block's 4-byte words into a
// caller-owned copy; it also transposes V's scales to [B][H][C/64][D], so that a block's D scales are one contiguous run).  The
// per-block K scales and V scales ride in the ring next to the codes, one 1 KiB request per stage.
// Requests are LDS-DMA (dma16) into XOR-swizzled stages; the stage two blocks ahead is requested in mid-iteration, behind the last
// ordinary load of the block (mask, scale map), so that no wait of the compiler's meets a fresh request.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_formats.h"
#include "qt_mx.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kBS = 64;                                   // block size of all four operands = keys per ring stage
constexpr int kMaxKeys = 16384;
constexpr int kRing = 3;
constexpr int kScaleBytes = 1024;                         // K scales [64][D/64], then V scales [D], fp32; the rest is padding

template <int D>
struct Stage {
    static constexpr int kCodes = kBS * D;                // K block [64 keys][D], V^T block [D][64 keys]
    static constexpr int kK = 0, kV = kCodes, kS = 2 * kCodes, kBytes = 2 * kCodes + kScaleBytes;
    static constexpr int kPieces = D / 64;                // 1 KiB request pieces per wave and operand
};

struct MxiAttnArgs {
    const int8_t *q, *k, *v;                              // v: the permuted copy
    const float *sq, *sk, *sv;                            // sv: the transposed copy
    const uint16_t *mask;
    long msb, msh, msq;
    uint16_t *out;
    int H, Q, C;
    float scaling;
    int div;
    float flo, fhi, quant_max;                            // P's quantizer
    int qmax_exp, pow2;
    const uint16_t *scale_lut;
};

// outstanding requests of this wave allowed to remain: n in 0 .. 5 (wave-uniform)
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    }
}

// offset of 16-byte chunk `chunk` of row `row` in a stage image: 128-byte rows (K at head_dim 128) and 64-byte rows (K at head_dim 64,
// V^T), the swizzles of qt_attention_fp8_long.hip
__device__ __forceinline__ int off128(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int off64(int row, int chunk) { return row * 64 + ((chunk ^ (((row >> 3) & 1) << 1)) << 4); }

template <int D>
__global__ __launch_bounds__(256, 2) void attention_mxi_kernel(MxiAttnArgs a) {
    using S = Stage<D>;
    constexpr int kNB = D / kBS;                          // 64-blocks of head_dim
    constexpr int kDT = D / 16;                           // output tiles of 16 d
    constexpr int kP = S::kPieces;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = l & 15, g = l >> 4;
    const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
    const int nkb = a.C / kBS;
    const int q0 = (int)blockIdx.y * 64;
    const int qrow = q0 + w * 16 + r, qc = min(qrow, a.Q - 1);      // rows >= Q re-read the last row and are never stored
    const uint32_t l0 = lds_addr(lds);

    // ---- request geometry: lane l of a piece lands at byte 16 l of it, so it fetches the chunk that the swizzle puts there
    const int8_t *kp[kP], *vp[kP];
#pragma unroll
    for (int i = 0; i < kP; ++i) {
        const int piece = w * kP + i;
        if (D == 128) {
            const int row = piece * 8 + (l >> 3);                   // key of the block
            kp[i] = a.k + ((long)bh * a.C + row) * D + (((l & 7) ^ ((row >> 1) & 7)) << 4);          // + kb * 64 * D
        } else {
            const int row = piece * 16 + (l >> 2);
            kp[i] = a.k + ((long)bh * a.C + row) * D + (((l & 3) ^ (((row >> 3) & 1) << 1)) << 4);
        }
        const int vrow = piece * 16 + (l >> 2);                     // d
        vp[i] = a.v + ((long)bh * D + vrow) * a.C + (((l & 3) ^ (((vrow >> 3) & 1) << 1)) << 4);    // + kb * 64
    }
    // the scale piece (wave 3): D / 4 lanes of K scales, D / 4 lanes of V scales; at head_dim 64 lanes 32 .. 63 repeat them into the padding
    constexpr int kHalf = D / 4;
    const int sidx = l % kHalf, spart = (l / kHalf) & 1;
    const float *sp = spart ? a.sv + (long)bh * nkb * D + 4 * sidx : a.sk + (long)bh * a.C * kNB + 4 * sidx;
    const long sstep = spart ? D : kBS * kNB;                       // floats per key block
    auto issue = [&](int kb, bool with_v) {                         // kb < nkb: inside every array
        const uint32_t dst = l0 + (kb % kRing) * S::kBytes;
#pragma unroll
        for (int i = 0; i < kP; ++i) dma16(kp[i] + (long)kb * kBS * D, dst + S::kK + (w * kP + i) * 1024);
        if (with_v) {
#pragma unroll
            for (int i = 0; i < kP; ++i) dma16(vp[i] + (long)kb * kBS, dst + S::kV + (w * kP + i) * 1024);
        }
        if (w == 3) dma16(sp + (long)kb * sstep, dst + S::kS);
    };
    const int per1 = kP + (w == 3), per2 = 2 * kP + (w == 3);       // this wave's requests per stage

    // ---- the query fragment and its scales
    const int8_t *qp = a.q + ((long)bh * a.Q + qc) * D;
    v4i qf[kNB];
    float sq[kNB];
#pragma unroll
    for (int blk = 0; blk < kNB; ++blk) {
        qf[blk] = *(const v4i *)(qp + blk * kBS + 16 * g);
        sq[blk] = a.sq[((long)bh * a.Q + qc) * kNB + blk];
    }
    const uint16_t *mrow = a.mask ? a.mask + b * a.msb + h * a.msh + (long)qc * a.msq + 4 * g : nullptr;
    wait_vm(0);                                                     // the compiler's waits for these must not meet the block requests

    // the 16 logits of block kb as bf16 values: lg[t][i] = key 64 kb + 16 t + 4 g + i
    auto block_logits = [&](const uint8_t *st, int kb, float (&lg)[4][4]) {
        const float *ss = (const float *)(st + S::kS);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            v4f sk[kNB];
            if constexpr (kNB == 1) {
                sk[0] = *(const v4f *)(ss + 16 * tt + 4 * g);
            } else {
                const v4f s01 = *(const v4f *)(ss + 2 * (16 * tt + 4 * g)), s23 = *(const v4f *)(ss + 2 * (16 * tt + 4 * g) + 4);
                sk[0] = v4f{s01[0], s01[2], s23[0], s23[2]};
                sk[1] = v4f{s01[1], s01[3], s23[1], s23[3]};
            }
#pragma unroll
            for (int blk = 0; blk < kNB; ++blk) {                   // ascending block order
                const int off = D == 128 ? off128(16 * tt + r, 4 * blk + g) : off64(16 * tt + r, g);
                const v4i kf = *(const v4i *)(st + S::kK + off);
                const v4i p = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf[blk], v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf((float)p[i], sq[blk] * sk[blk][i], acc[i]);
            }
            uint2 mk = {0u, 0u};
            if (mrow) mk = *(const uint2 *)(mrow + kb * kBS + 16 * tt);
            const float mv[4] = {bf_lo(mk.x), bf_hi(mk.x), bf_lo(mk.y), bf_hi(mk.y)};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = bf16_round(acc[i]);
                v = a.div ? bf16_round(v / a.scaling) : bf16_round(v * a.scaling);
                if (mrow) v = bf16_round(v + mv[i]);
                lg[tt][i] = v;
            }
        }
    };

    const float kLog2e = 1.4426950408889634f;
    float lg[4][4];
    float m = -INFINITY, lsum = 0.0f;

    // ---- sweep 1: the row maximum and the sum of exponentials.  Block kb lives in stage kb % 3; block kb + 2 is requested in iteration
    // kb, behind its barrier -- everyone is through block kb - 1, that stage's last.
    issue(0, false);
    if (nkb > 1) issue(1, false);
    for (int kb = 0; kb < nkb; ++kb) {
        wait_vm(kb + 1 < nkb ? per1 : 0);
        __builtin_amdgcn_s_barrier();
        block_logits(lds + (kb % kRing) * S::kBytes, kb, lg);
        if (kb + 2 < nkb) issue(kb + 2, false);
        float bm = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) bm = fmaxf(fmaxf(fmaxf(bm, lg[tt][0]), fmaxf(lg[tt][1], lg[tt][2])), lg[tt][3]);
        bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float mn = fmaxf(m, bm);
        const float ref = mn == -INFINITY ? 0.0f : mn;              // only -inf logits so far: every term is 0, not inf - inf
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            s0 += __builtin_amdgcn_exp2f((lg[tt][0] - ref) * kLog2e);
            s1 += __builtin_amdgcn_exp2f((lg[tt][1] - ref) * kLog2e);
            s0 += __builtin_amdgcn_exp2f((lg[tt][2] - ref) * kLog2e);
            s1 += __builtin_amdgcn_exp2f((lg[tt][3] - ref) * kLog2e);
        }
        lsum = lsum * __builtin_amdgcn_exp2f((m - ref) * kLog2e) + (s0 + s1);
        m = mn;
    }
    __builtin_amdgcn_s_barrier();                                   // everyone is through sweep 1 (no request is outstanding)
    issue(0, true);
    if (nkb > 1) issue(1, true);
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = 1.0f / lsum;
    const bool row_nan = !(lsum >= 1.0f);                           // all -inf, or a NaN / +inf logit: torch's row is NaN
    const float mref = m == -INFINITY ? 0.0f : m;

    // ---- sweep 2: the same logits, the probabilities, their block quantizer, P.V
    v4f acc[kDT];
#pragma unroll
    for (int i = 0; i < kDT; ++i) acc[i] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nkb; ++kb) {
        wait_vm(kb + 1 < nkb ? per2 : 0);
        __builtin_amdgcn_s_barrier();
        const uint8_t *st = lds + (kb % kRing) * S::kBytes;
        block_logits(st, kb, lg);
        // probabilities as bf16 pairs, and the block amax of the row on their bit patterns (not negative; NaN patterns win)
        uint32_t pw[4][2], am = 0;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            float p[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) p[i] = __builtin_amdgcn_exp2f((lg[tt][i] - mref) * kLog2e) * inv;
            pw[tt][0] = pack_bf16x2(p[0], p[1]);
            pw[tt][1] = pack_bf16x2(p[2], p[3]);
            am = pk_max_u16(am, pk_max_u16(pw[tt][0] & 0x7FFF7FFFu, pw[tt][1] & 0x7FFF7FFFu));
        }
        am = max(am & 0xFFFFu, am >> 16);
        am = max(am, (uint32_t)__shfl_xor((int)am, 16, 64));
        am = max(am, (uint32_t)__shfl_xor((int)am, 32, 64));
        const qt_mx::BlockScale sc = qt_mx::block_scale<kIoBf16>(am << 16, a.pow2 != 0, a.quant_max, a.qmax_exp, a.scale_lut);
        const float s = sc.s, rcp = sc.recip();
        const bool recip_ok = sc.recip_ok();
        asm volatile("" ::"v"(s), "v"(rcp));                       // the scale map's gather is consumed in front of the request
        if (kb + 2 < nkb) issue(kb + 2, true);
        // the element step of quantize_mx_kernel: map(bf16(p / s)), the map being intN's closed form; a NaN has code 0 (the row is NaN)
        v4i pf;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float x0 = bf_lo(pw[tt][j]), x1 = bf_hi(pw[tt][j]);
                const uint32_t qw = recip_ok ? pack_bf16x2(x0 * rcp, x1 * rcp) : pack_bf16x2(x0 / s, x1 / s);
                const float v0 = qt_u2f(qt_int_img(qw << 16, a.flo, a.fhi)), v1 = qt_u2f(qt_int_img(qw & 0xFFFF0000u, a.flo, a.fhi));
                const int c0 = v0 != v0 ? 0 : (int)v0, c1 = v1 != v1 ? 0 : (int)v1;
                word |= ((uint32_t)(uint8_t)c0 << (16 * j)) | ((uint32_t)(uint8_t)c1 << (16 * j + 8));
            }
            pf[tt] = (int)word;
        }
        const float *sv = (const float *)(st + S::kS) + kBS * kNB;
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) {
            const v4i vf = *(const v4i *)(st + S::kV + off64(16 * dt + r, g));
            const v4f svd = *(const v4f *)(sv + 16 * dt + 4 * g);
            const v4i pi = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pf, v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[dt][i] = __builtin_fmaf((float)pi[i], s * svd[i], acc[dt][i]);
        }
    }
    // ---- lane (r, g) holds query r, d = 16 dt + 4 g + {0..3}: one 8-byte store per tile
    if (qrow < a.Q) {
        uint8_t *orow = (uint8_t *)a.out + ((long)bh * a.Q + qrow) * (2 * D) + 8 * g;
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) {
            uint2 o = {pack_bf16x2(acc[dt][0], acc[dt][1]), pack_bf16x2(acc[dt][2], acc[dt][3])};
            if (row_nan) o = uint2{0x7FC07FC0u, 0x7FC07FC0u};
            *(uint2 *)(orow + dt * 32) = o;
        }
    }
}

// The prepare launch.  One thread per (b h, d, key block): the block's sixteen 4-byte words of V^T's code row transposed 4 x 4 -- word
// 4 g + t of the copy is word 4 t + g, so byte 16 g + 4 t + i is key 16 t + 4 g + i -- and the block's scale moved to [b h][block][d].
__global__ __launch_bounds__(256) void mxi_attention_prepare_kernel(const int8_t *v, const float *sv, int8_t *vperm, float *svt, long total,
                                                                   int D, int nkb) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int kb = (int)(i % nkb);
    const long row = i / nkb;                             // b h D + d
    const int d = (int)(row % D);
    const long bh = row / D;
    const uint4 *src = (const uint4 *)(v + i * kBS);
    const uint4 w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3];
    uint4 *dst = (uint4 *)(vperm + i * kBS);
    dst[0] = uint4{w0.x, w1.x, w2.x, w3.x};
    dst[1] = uint4{w0.y, w1.y, w2.y, w3.y};
    dst[2] = uint4{w0.z, w1.z, w2.z, w3.z};
    dst[3] = uint4{w0.w, w1.w, w2.w, w3.w};
    svt[(bh * nkb + kb) * D + d] = sv[i];
}

template <int D>
int launch_mxi_attention(const MxiAttnArgs &a, long BH, hipStream_t st) {
    constexpr int kLds = kRing * Stage<D>::kBytes;                  // 51 KiB at head_dim 128, 27 KiB at 64
    if (const int rc = qt_allow_lds<attention_mxi_kernel<D>>(kLds)) return rc;
    attention_mxi_kernel<D><<<dim3((unsigned)BH, (unsigned)((a.Q + 63) / 64)), 256, kLds, st>>>(a);
    return qt_launch_status();
}

}  // namespace

extern "C" int qt_attention_mxi(const int8_t *q_codes, const float *q_scales, const int8_t *k_codes, const float *k_scales, const int8_t *v_codes,
                                const float *v_scales, int8_t *v_work, float *v_scales_work, const uint16_t *mask_dev, long mask_sb, long mask_sh,
                                long mask_sq, float scaling, int scaling_is_div, const qt_format *p_format, float quant_max,
                                int force_scale_power_of_two, const uint16_t *scale_map_dev, uint16_t *out_dev, long B, int H, int Q, int C,
                                int head_dim, int block_size, void *stream) {
    if (!q_codes || !q_scales || !k_codes || !k_scales || !v_codes || !v_scales || !v_work || !v_scales_work || !out_dev || !p_format)
        return QT_ERR_BAD_ARG;
    if (B < 0 || H < 1 || Q < 0 || block_size != kBS || (head_dim != 64 && head_dim != 128) || C < kBS || C % kBS != 0 || C > kMaxKeys ||
        B * H > 65535 || (Q + 63) / 64 > 65535)
        return QT_ERR_BAD_ARG;
    // P's element format: intN, N <= 8, in closed form
    if (p_format->kind != QT_FMT_INT || !(p_format->flo >= -128.0f) || !(p_format->fhi <= 127.0f) || !(p_format->flo <= p_format->fhi) ||
        p_format->flo != truncf(p_format->flo) || p_format->fhi != truncf(p_format->fhi))
        return QT_ERR_BAD_ARG;
    if (!(quant_max > 0.0f) || !(quant_max < INFINITY) || !(scaling == scaling) || (scaling_is_div != 0 && scaling_is_div != 1))
        return QT_ERR_BAD_ARG;
    if (force_scale_power_of_two && scale_map_dev) return QT_ERR_BAD_ARG;                      // calculate_mx_qparam applies the map to amax / qmax only
    if (B * H * Q == 0) return QT_OK;
    if ((((uintptr_t)q_codes | (uintptr_t)k_codes | (uintptr_t)v_codes | (uintptr_t)v_work | (uintptr_t)k_scales | (uintptr_t)v_scales_work) & 15u) ||
        (((uintptr_t)q_scales | (uintptr_t)v_scales) & 3u) || ((uintptr_t)out_dev & 7u) || ((uintptr_t)scale_map_dev & 1u) ||
        (mask_dev && (((uintptr_t)mask_dev & 7u) || ((mask_sb | mask_sh | mask_sq) & 3))))
        return QT_ERR_UNALIGNED;
    hipStream_t st = (hipStream_t)stream;
    const int nkb = C / kBS;
    const long total = B * H * head_dim * nkb;
    mxi_attention_prepare_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(v_codes, v_scales, v_work, v_scales_work, total, head_dim, nkb);
    if (const int rc = qt_launch_status()) return rc;
    int qe = 0;
    (void)frexpf(quant_max, &qe);                                   // floor(log2(quant_max)) = qe - 1, as the quantize_mx launch derives it
    MxiAttnArgs a{q_codes, k_codes, v_work, q_scales, k_scales, v_scales_work, mask_dev, mask_sb, mask_sh, mask_sq, out_dev, H, Q, C, scaling,
                  scaling_is_div, p_format->flo, p_format->fhi, quant_max, qe - 1, force_scale_power_of_two ? 1 : 0, scale_map_dev};
    return head_dim == 128 ? launch_mxi_attention<128>(a, B * H, st) : launch_mxi_attention<64>(a, B * H, st);
}
