// qt_attention_fp8_d32.hip -- the attention core on FP8 codes at head_dim 32 (MobileBERT: 4 heads of 32, at most 512 positions):
// Q.K^T, scaling, mask, softmax, fake-quant of the probabilities and P.V in ONE launch, the S x S tensors never written.
//
// Replaces, when all four fake-quantizers around the two matmuls are stateless E4M3 / E5M2 ones (unit scale),
//     av_matmul(fq_p(softmax(attn_scaling(qk_matmul(fq_q(q), fq_k(k)^T), scale) + mask)), fq_v(v))
//                                                     modules/quantizable/modeling_mobilebert.py:80-93
// with the module chain's rounding points kept, exactly as qt_attention_fp8 keeps them: scores rounded to bf16, bf16(score * scaling),
// bf16(. + mask), softmax in fp32 over the WHOLE row (no running rescale), probabilities rounded to bf16, their fake-quantizer (the
// hardware conversion), P.V accumulated in fp32, output bf16, the consumer's FP8 fake-quantizer on the way out.
//
// Padding 32 up to the 128-deep scaled instruction (as head_dim 64 pads to it) would multiply three quarters zeros; 32 is exactly the
// depth of v_mfma_f32_16x16x32_fp8_fp8 / _bf8_bf8, so Q.K^T is one of those per 16 x 16 tile.  And a head is small: its whole K (Sk x 32
// bytes) and V^T (32 x Sk bytes) are 32 KiB at 512 keys, so both are requested ONCE by LDS-DMA, K first, and stay in LDS for the life of
// the workgroup -- no ring, no double buffer, two barriers before the epilogue: K is waited for before sweep 1, V^T only after the
// exponentials, before sweep 2.
//
// A workgroup = 4 waves owns 64 query rows of one (batch, head); a wave owns 16 of them against ALL keys: its 16 x Sk strip is at most
// 128 fp32 registers a lane, so the keys are not split between wave groups, no row statistics or partial P.V sums meet in LDS, and each
// exponential is evaluated once.  The operands are multiplied swapped (K fragment first): lane (r, g) holds query r against keys
// 16 t + 4 g + {0..3} of every tile t -- the ownership of the other two kernels and of qt_value_codes.h -- so the row statistics are
// lane-local plus two shuffles (score_half, qt_attention_fp8_core.h, with the 32-deep instruction), and the lane's 32 probability codes
// of a 128-key block ARE the B operand of one v_mfma_scale_f32_16x16x128_f8f6f4 (unit scales) per 16 columns of head_dim: two of them,
// 8 accumulator registers.  Key blocks beyond every row's extent are neither requested nor multiplied; a wave skips the half-blocks
// beyond its own 16 rows.
//
// The LDS images.  K: a 16-key tile is 512 bytes; lane (r, g) needs bytes 8 g .. 8 g + 7 of key r (ds_read_b64).  Left as rows of 32
// bytes, keys r and r + 8 of the 32 lanes a ds_read_b64 serves at a time (g = 0, 1: 16 bytes of each of 16 rows, 32 bytes apart) would meet
// in the same banks.  So the DMA, whose unit is 16 bytes, lays the tile down as [half h][key r][16 bytes]: lane (r, g) reads at
// 256 (g >> 1) + 16 r + 8 (g & 1), lanes 0-31 cover 256 contiguous bytes = each of the 64 banks once, lanes 32-63 the next 256.
// V^T: rows of 128 bytes (the keys of a block, in the k-slot order qt_value_codes_t_d32 writes), 16-byte chunks XOR-swizzled by the row
// (chunk_off) as in the other two kernels: the 16 lanes a ds_read_b128 serves at a time (one g, r = 0..15) read chunk g ^ (r >> 1) of
// rows r -- eight chunk slots x two rows 128 bytes apart = 64 banks, each once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_attention_fp8_core.h"
#include "qt_value_codes.h"

namespace {

constexpr int kD = 32, kDT = kD / 16;                                      // head_dim; output tiles of 16 d
constexpr int kBuf = kBlock * kD;                                          // one K / V^T block of codes: 4 KiB = one 1 KiB piece per wave
constexpr int kMaxBlocksD32 = 4;                                           // 512 keys

// all but the latest n (wave-uniform, 0 .. 4) of this wave's LDS-DMA requests have arrived
__device__ __forceinline__ void wait_dma_but(int n) {
    if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (n == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (n == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if (n == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// F: operand format of q, k, v and p (0 = E4M3, 1 = E5M2).  MB: key blocks of 128 the strip is sized for (4: up to 512 keys, two workgroups
// a CU; 2 and 1: 256 and 128 keys -- half and a quarter of the strip registers and of the LDS, so three and four workgroups share a CU)
template <int F, int MB>
__global__ __launch_bounds__(256, MB == 4 ? 2 : MB == 2 ? 3 : 4) void attention_fp8_d32_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];          // K image (Sk x 32 bytes), then V^T image (Sk / 128 blocks of 32 x 128)
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = l & 15, g = l >> 4;
    const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
    const int nkb = a.Sk / kBlock, nqb = (a.Sq + 63) / 64;
    const int qb = nqb - 1 - (int)blockIdx.y;                              // the heaviest blocks of rows of every head first under a causal mask
    const int q0 = qb * 64;
    const int qrow = q0 + w * 16 + r, qc = min(qrow, a.Sq - 1);
    int nlive, wmax, wmin, my_live;                                        // the row extents: split_row_extents
    split_row_extents(a, b, h, q0, qc, l, nkb, nlive, wmax, wmin, my_live);
    const bool simple = a.mask && a.row_live && (a.mask_simple || (a.mask_irregular && *a.mask_irregular == 0)), full = a.mask && !simple;
    if (!simple) wmin = a.Sk;                                              // extents then only bound the walk; inside them the mask is read
    if (!simple && !a.row_live) wmax = a.Sk;
    const uint8_t *qp = a.q8 + ((long)bh * a.Sq + qc) * kD;
    const uint2 q2 = *(const uint2 *)(qp + 8 * g);
    const uint16_t *mrow = full ? a.mask + b * a.msb + h * a.msh + (long)qc * a.msq + 4 * g : nullptr;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the compiler's waits for these must not meet the block requests
    // DMA: a block is 4 pieces of 1 KiB, wave w requests piece w of every live block.  K piece: 32 keys = two tiles, lane = (tile, half,
    // key) in that order (the image above); V^T piece: 8 rows (d) x 128 bytes, chunks swizzled by the row.  kb < nlive <= nkb: inside k8 / vt8.
    const uint32_t k0 = lds_addr(lds) + w * 1024, v0 = k0 + a.Sk * kD;
    const uint8_t *kp = a.k8 + ((long)bh * a.Sk + w * 32 + (l >> 5) * 16 + (l & 15)) * kD + ((l >> 4) & 1) * 16;          // + block * 128 * 32
    const int vrow = w * 8 + (l >> 3);
    const uint8_t *vp = a.vt8 + ((long)bh * kD + vrow) * a.Sk + (((l & 7) ^ ((vrow >> 1) & 7)) << 4);                     // + block * 128
#pragma unroll
    for (int kb = 0; kb < MB; ++kb)
        if (kb < nlive) dma16(kp + kb * kBuf, k0 + kb * kBuf);
#pragma unroll
    for (int kb = 0; kb < MB; ++kb)
        if (kb < nlive) dma16(vp + kb * kBlock, v0 + kb * kBuf);
    const v8i qf = {(int)q2.x, (int)q2.y, 0, 0, 0, 0, 0, 0};               // (score_half's operand type: the 32-deep instruction takes the first two words)
    const int f_k = 256 * (g >> 1) + 16 * r + 8 * (g & 1);
    const int f_v0 = chunk_off(r, g), f_v1 = chunk_off(r, 4 + g);          // V^T: tiles 0-3 and 4-7 of the block are one 16-byte chunk each
    // how many of the four tiles of half c of block kb does one of this wave's rows reach?
    auto tiles_of = [&](int kb, int c) { return min(4, max(0, (wmax - (kb * kBlock + 64 * c) + 15) >> 4)); };

    float e[MB][8][4];                                                     // this wave's strip: logits, then their exponentials
    float mx = -INFINITY;
    // ---- sweep 1: scores.  K is here when all but the nlive V^T requests have arrived
    wait_dma_but(nlive);
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int kb = 0; kb < MB; ++kb) {
        if (kb < nlive) {
            const uint8_t *blk = lds + kb * kBuf;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int key0 = kb * kBlock + 64 * c, nt = tiles_of(kb, c);
                float (*ev)[4] = &e[kb][4 * c];
                if (nt == 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) ev[j][0] = ev[j][1] = ev[j][2] = ev[j][3] = -INFINITY;
                } else if (full) {
                    score_half<F, kD, 2>(blk, 4 * c, qf, f_k, 0, a.scaling, ev, mx, mrow, key0, 0, 4);
                } else if (!simple || key0 + 64 <= wmin) {
                    score_half<F, kD, 0>(blk, 4 * c, qf, f_k, 0, a.scaling, ev, mx, nullptr, key0, 0, 4);
                } else {
                    score_half<F, kD, 1>(blk, 4 * c, qf, f_k, 0, a.scaling, ev, mx, nullptr, key0 + 4 * g, my_live, nt);
                }
            }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // ---- exponentials, once (a column at the bf16 minimum, or beyond the extents, gives exactly 0)
    const float kLog2e = 1.4426950408889634f;                              // (v - max) first: a fully masked row has max = the bf16 minimum
    float2_t sum2 = {0.0f, 0.0f};
#pragma unroll
    for (int kb = 0; kb < MB; ++kb) {
        if (kb < nlive) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (tiles_of(kb, c) != 0) {
#pragma unroll
                    for (int j = 4 * c; j < 4 * c + 4; ++j) {
                        float *v = e[kb][j];
                        const float2_t a0 = (float2_t{v[0], v[1]} - float2_t{mx, mx}) * float2_t{kLog2e, kLog2e};
                        const float2_t a1 = (float2_t{v[2], v[3]} - float2_t{mx, mx}) * float2_t{kLog2e, kLog2e};
                        v[0] = __builtin_amdgcn_exp2f(a0[0]); v[1] = __builtin_amdgcn_exp2f(a0[1]);
                        v[2] = __builtin_amdgcn_exp2f(a1[0]); v[3] = __builtin_amdgcn_exp2f(a1[1]);
                        sum2 += float2_t{v[0], v[1]};
                        sum2 += float2_t{v[2], v[3]};
                    }
                }
            }
        }
    }
    float sum = sum2[0] + sum2[1];
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    // ---- sweep 2: the probabilities' codes, P.V.  V^T is waited for only now
    v4f acc[kDT];
#pragma unroll
    for (int i = 0; i < kDT; ++i) acc[i] = v4f{0.f, 0.f, 0.f, 0.f};
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int kb = 0; kb < MB; ++kb) {
        if (kb < nlive) {
            const bool live0 = tiles_of(kb, 0) != 0, live1 = tiles_of(kb, 1) != 0;
            if (live0 | live1) {
                const uint8_t *vblk = lds + a.Sk * kD + kb * kBuf;
                u32x4 vlo[kDT], vhi[kDT];
#pragma unroll
                for (int dt = 0; dt < kDT; ++dt) {                           // requested before the codes are formed
                    vlo[dt] = *(const u32x4 *)(vblk + dt * 2048 + f_v0);
                    vhi[dt] = *(const u32x4 *)(vblk + dt * 2048 + f_v1);
                }
                uint32_t pd[8];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (c == 0 ? live0 : live1) {
#pragma unroll
                        for (int j = 4 * c; j < 4 * c + 4; ++j) {
                            const float *v = e[kb][j];
                            const uint32_t p0 = pack_bf16x2(v[0] * inv, v[1] * inv), p1 = pack_bf16x2(v[2] * inv, v[3] * inv);   // probabilities, bf16
                            pd[j] = prob_codes<F == 1>(p0, p1);                                                               // fq_p
                        }
                    } else {
                        pd[4 * c] = pd[4 * c + 1] = pd[4 * c + 2] = pd[4 * c + 3] = 0;
                    }
                }
                const v8i pf = {(int)pd[0], (int)pd[1], (int)pd[2], (int)pd[3], (int)pd[4], (int)pd[5], (int)pd[6], (int)pd[7]};
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int dt = 0; dt < kDT; ++dt) {
                    const v8i vf = {(int)vlo[dt].x, (int)vlo[dt].y, (int)vlo[dt].z, (int)vlo[dt].w, (int)vhi[dt].x, (int)vhi[dt].y, (int)vhi[dt].z, (int)vhi[dt].w};
                    acc[dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf, acc[dt], F, F, 0, kUnit, 0, kUnit);
                }
            }
        }
    }
    // ---- the finished 64 x 32 tile leaves through LDS (8 KiB: Sk = 128 gives exactly that): every wave rounds its own 16 rows -- bf16
    // values when they are wanted, codes when they are -- into the operand images, which are dead by now, and then the waves store 16
    // bytes a lane: rows of 64 bytes of `out`, of 32 bytes of `out8`
    const int prow = w * 16 + r;
    uint8_t *tile_v = lds, *tile_c = lds + 64 * kValRow<kD>;
    __syncthreads();                                                       // everyone is through sweep 2
    {
        uint8_t *vrow8 = tile_v + prow * kValRow<kD> + 8 * g, *crow = tile_c + prow * kCodeRow<kD> + 4 * g;       // this lane's columns 16 dt + 4 g ..
        uint32_t o[4] = {pack_bf16x2(acc[0][0], acc[0][1]), pack_bf16x2(acc[0][2], acc[0][3]), pack_bf16x2(acc[1][0], acc[1][1]),
                         pack_bf16x2(acc[1][2], acc[1][3])};
        if (a.out8) {
            const uint2 codes = a.out_fmt.p0 == 2 ? fq8_hw_vec8<true>(o, a.out_fmt) : fq8_hw_vec8<false>(o, a.out_fmt);
            *(uint32_t *)crow = codes.x;
            *(uint32_t *)(crow + 16) = codes.y;
        }
        if (a.out) {
            *(uint2 *)vrow8 = uint2{o[0], o[1]};
            *(uint2 *)(vrow8 + 32) = uint2{o[2], o[3]};
        }
    }
    __syncthreads();
    const int rows = min(64, a.Sq - q0);                                   // rows >= Sq are never stored
    const long orow0 = ((long)b * a.Sq + q0) * a.H + h;                    // row q0 of this head, in rows of 32 elements; the next is H further
    if (a.out) {
        const int row = t >> 2, ch = t & 3;                                // 64 rows x 4 chunks of 16 bytes: one a lane
        if (row < rows) *(u32x4 *)((uint8_t *)a.out + (orow0 + (long)row * a.H) * (2 * kD) + 16 * ch) = *(const u32x4 *)(tile_v + row * kValRow<kD> + 16 * ch);
    }
    if (a.out8 && t < 128) {
        const int row = t >> 1, ch = t & 1;                                // 64 rows x 2 chunks
        if (row < rows) *(u32x4 *)(a.out8 + (orow0 + (long)row * a.H) * kD + 16 * ch) = *(const u32x4 *)(tile_c + row * kCodeRow<kD> + 16 * ch);
    }
}

// fq_v(V) as FP8 codes in the layout the P.V instruction wants: qt_value_codes.h.  One workgroup per (batch * head, key block).
template <bool E5M2>
__global__ __launch_bounds__(256) void value_codes_t_d32_kernel(const uint16_t *v, uint8_t *vt8, int H, long Sk, long sb, long sh, long sk, qt_format fmt) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kD * kBlock];
    value_codes_block<E5M2, kD>(tile, v, vt8, (int)blockIdx.x, (long)blockIdx.y, H, Sk, sb, sh, sk, fmt);
}

template <int F, int MB>
int launch_d32_mb(const AttnArgs &a, long BH, int nqb, hipStream_t st) {
    static_assert(kBlock * 2 * kD >= 64 * (kValRow<kD> + kCodeRow<kD>), "the finished tile reuses the operand images, at one key block too");
    attention_fp8_d32_kernel<F, MB><<<dim3((unsigned)BH, (unsigned)nqb), 256, a.Sk * 2 * kD, st>>>(a);       // at most 32 KiB: no opt-in needed
    return qt_launch_status();
}

template <int F>
int launch_d32(const AttnArgs &a, long BH, int nqb, hipStream_t st) {
    if (a.Sk <= kBlock) return launch_d32_mb<F, 1>(a, BH, nqb, st);
    if (a.Sk <= 2 * kBlock) return launch_d32_mb<F, 2>(a, BH, nqb, st);
    return launch_d32_mb<F, 4>(a, BH, nqb, st);
}

}  // namespace

extern "C" {

int qt_value_codes_t_d32(const uint16_t *v_dev, uint8_t *vt8_dev, long B, long H, long Sk, long stride_b, long stride_h, long stride_k,
                         const qt_format *fmt, void *stream) {
    if (B * H * Sk == 0) return QT_OK;
    const int f8 = qt_fp8_code(fmt);
    if (!v_dev || !vt8_dev || B < 0 || H < 1 || Sk < 0 || Sk % kBlock != 0 || B * H > 65535 || !f8) return QT_ERR_BAD_ARG;
    if ((((uintptr_t)v_dev | (uintptr_t)vt8_dev) & 15u) || ((stride_b | stride_h | stride_k) & 7)) return QT_ERR_UNALIGNED;
    const dim3 grid((unsigned)(Sk / kBlock), (unsigned)(B * H));
    hipStream_t st = (hipStream_t)stream;
    if (f8 == 2) value_codes_t_d32_kernel<true><<<grid, 256, 0, st>>>(v_dev, vt8_dev, (int)H, Sk, stride_b, stride_h, stride_k, *fmt);
    else value_codes_t_d32_kernel<false><<<grid, 256, 0, st>>>(v_dev, vt8_dev, (int)H, Sk, stride_b, stride_h, stride_k, *fmt);
    return qt_launch_status();
}

int qt_attention_fp8_d32(const uint8_t *q8_dev, const uint8_t *k8_dev, const uint8_t *vt8_dev, int operand_format, const uint16_t *mask_dev,
                         long mask_sb, long mask_sh, long mask_sq, const int *row_live_dev, long live_sb, long live_sh, long live_sq,
                         int mask_is_simple, const int *mask_irregular_dev, uint16_t *out_dev, uint8_t *out8_dev, const qt_format *out_format, long B,
                         int H, int Sq, int Sk, int head_dim, float scaling, void *stream) {
    if (B * H * Sq == 0) return QT_OK;
    if (!q8_dev || !k8_dev || !vt8_dev || (!out_dev && !out8_dev) || B < 0 || H < 1 || Sq < 1 || Sk < kBlock || Sk % kBlock != 0 ||
        Sk > kBlock * kMaxBlocksD32 || B * H > 65535 || operand_format < 0 || operand_format > 1 || head_dim != kD)
        return QT_ERR_BAD_ARG;
    if ((((uintptr_t)q8_dev | (uintptr_t)k8_dev | (uintptr_t)vt8_dev) & 15u) || ((uintptr_t)out_dev & 15u) ||
        (mask_dev && ((((uintptr_t)mask_dev) & 7u) || ((mask_sb | mask_sh | mask_sq) & 3))))
        return QT_ERR_UNALIGNED;
    if (out8_dev && !qt_fp8_code(out_format)) return QT_ERR_BAD_ARG;
    if ((uintptr_t)out8_dev & 15u) return QT_ERR_UNALIGNED;                 // both results leave in 16-byte stores
    AttnArgs a{q8_dev, k8_dev, vt8_dev, mask_dev, mask_sb, mask_sh, mask_sq, row_live_dev, live_sb, live_sh, live_sq, mask_is_simple ? 1 : 0,
               out_dev, H, Sq, Sk, scaling, out8_dev, out8_dev ? *out_format : qt_format{}, mask_irregular_dev};
    const int nqb = (Sq + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    return operand_format == 0 ? launch_d32<0>(a, B * H, nqb, st) : launch_d32<1>(a, B * H, nqb, st);
}

}  // extern "C"
