// qt_attention_fp8_ragged.hip -- the attention core on FP8 codes at ANY key count from 1 to 512 (head_dim 64 / 128): a batch padded to its
// longest sample (GLUE / SQuAD without --pad_to_max_length: 77, 136, 200 keys), a last partial batch, ViT's 197 tokens.  Q.K^T, scaling,
// mask, softmax, fake-quant of the probabilities and P.V in ONE launch, the S x S tensors never written.
//
// Replaces, when all four fake-quantizers around the two matmuls are stateless E4M3 / E5M2 ones (unit scale),
//     av_matmul(fq_p(softmax(attn_scaling(qk_matmul(fq_q(q), fq_k(k)^T), scale) + mask)), fq_v(v))
//                                                     modules/quantizable/modeling_bert.py:118-158
// with the module chain's rounding points kept, exactly as qt_attention_fp8 keeps them: scores rounded to bf16, bf16(score * scaling),
// bf16(. + mask), softmax in fp32 over the WHOLE row (no running rescale), probabilities rounded to bf16, their fake-quantizer (the
// hardware conversion), P.V accumulated in fp32, output bf16, the consumer's FP8 fake-quantizer on the way out.
//
// The shape of attention_fp8_d32_kernel: a workgroup = 4 waves owns 64 query rows of one (batch, head); a wave owns 16 of them against ALL
// keys -- its 16 x Skp strip is at most 128 fp32 registers a lane -- so no row statistics or partial sums meet in LDS and each exponential
// is evaluated once.  Lane (r, g) holds query r against keys 16 t + 4 g + {0..3} of every tile t (score_half, qt_attention_fp8_core.h); its
// 32 probability codes of a 128-key block are the B operand of one v_mfma_scale_f32_16x16x128_f8f6f4 per 16 columns of head_dim.  The
// head's K and V^T are requested once by LDS-DMA, K first, in the images of attention_fp8_split_kernel (128-byte rows: chunk_off; the
// 64-byte rows of head_dim 64: chunk c of row r in slot c ^ 2 (r >> 3 & 1)); K is waited for before sweep 1, V^T only after the
// exponentials.  At head_dim 128 beyond 256 keys the two images would be 96 / 128 KiB -- one workgroup, four waves, a CU -- so there V^T
// is requested after sweep 1 INTO K's place (64 KiB, two workgroups a CU: the other workgroup's arithmetic covers the wait, which one
// workgroup's own exponentials would not).
//
// The tail.  Skp = 128 ceil(Sk / 128).  K: the DMA's source rows of keys >= Sk are clamped to key Sk - 1 -- inside this head's k8, whatever
// follows it -- and what they score is discarded: every column >= Sk gets the logit -inf unconditionally, before the row maximum (score_half's
// tail modes), so its exponential and its probability code are exactly 0 and a fully masked row is uniform over the Sk real keys.  V^T
// (qt_value_codes_t_ragged) has rows of Skp bytes -- 16-byte aligned for the DMA at any Sk -- and code 0 in every slot of a key >= Sk:
// 0 x 0, never 0 x a NaN code.  The mask is read element by element (2-byte loads: its rows may start at any even address), never at a
// column >= Sk.  Tiles and half-blocks wholly beyond Sk are skipped as those beyond a wave's row extents are (wmax <= Sk).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_attention_fp8_core.h"

namespace {

constexpr int kMaxBlocksRagged = 4;                                        // 512 keys

// all of this wave's LDS-DMA requests but the latest PER * n (n wave-uniform, 0 .. 4) have arrived
template <int PER>
__device__ __forceinline__ void wait_dma_but_blocks(int n) {
    if (n >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * PER) : "memory");
    else if (n == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * PER) : "memory");
    else if (n == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory");
    else if (n == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// does V^T take K's place in LDS (requested after sweep 1)?  head_dim 128 beyond 256 keys: see the head of the file
template <int D, int MB> constexpr bool kShare = D == 128 && MB == 4;

// workgroups a CU the registers are budgeted for: what the LDS images allow (64 KiB at MB = 4 and at head_dim 128 / MB = 2: two), else
// the d32 kernel's three and four
template <int D, int MB> constexpr int kWgPerCu = (MB == 4 || (D == 128 && MB == 2)) ? 2 : MB == 2 ? 3 : 4;

// F: operand format of q, k, v and p (0 = E4M3, 1 = E5M2).  MB: key blocks of 128 the strip is sized for (4, 2, 1: up to 512, 256, 128 keys)
template <int F, int D, int MB>
__global__ __launch_bounds__(256, (kWgPerCu<D, MB>)) void attention_fp8_ragged_kernel(AttnArgs a) {
    constexpr int kBuf = kBlock * D;                                       // one K / V^T block of codes: 16 KiB at head_dim 128, 8 KiB at 64
    constexpr int kPP = D / 32;                                            // 1 KiB request pieces per wave and block
    constexpr int kDT = D / 16;                                            // output tiles of 16 d
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];          // K image (nkb blocks), then -- or, kShare, in its place -- the V^T image
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = l & 15, g = l >> 4;
    const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
    const int nkb = (a.Sk + kBlock - 1) / kBlock, skp = nkb * kBlock, nqb = (a.Sq + 63) / 64;
    const int qb = nqb - 1 - (int)blockIdx.y;                              // the heaviest blocks of rows of every head first under a causal mask
    const int q0 = qb * 64;
    const int qrow = q0 + w * 16 + r, qc = min(qrow, a.Sq - 1);
    int nlive, wmax, wmin, my_live;                                        // the row extents: split_row_extents (entries in [0, Sk]; wmax <= Sk)
    split_row_extents(a, b, h, q0, qc, l, nkb, nlive, wmax, wmin, my_live);
    const bool simple = a.mask && a.row_live && (a.mask_simple || (a.mask_irregular && *a.mask_irregular == 0)), full = a.mask && !simple;
    if (!simple) wmin = a.Sk;                                              // extents then only bound the walk; inside them the mask is read
    if (!simple && !a.row_live) wmax = a.Sk;
    const uint8_t *qp = a.q8 + ((long)bh * a.Sq + qc) * D;
    const u32x4 qlo = *(const u32x4 *)(qp + 16 * g), qhi = D == 128 ? *(const u32x4 *)(qp + 64 + 16 * g) : u32x4{0u, 0u, 0u, 0u};
    const uint16_t *mrow = full ? a.mask + b * a.msb + h * a.msh + (long)qc * a.msq + 4 * g : nullptr;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the compiler's waits for these must not meet the block requests
    // DMA: a block is D / 8 pieces of 1 KiB, wave w requests pieces kPP w .. kPP w + kPP - 1 of every live block (kb < nlive <= nkb).
    // K piece, head_dim 128: 8 key rows x 128 bytes, chunks swizzled by the row; head_dim 64: 16 key rows x 64 bytes.  A row >= Sk is
    // fetched from row Sk - 1.  V^T piece: 8 rows (d) x 128 bytes of a row of skp: always inside vt8.
    const uint32_t k0 = lds_addr(lds), v0 = kShare<D, MB> ? k0 : k0 + nkb * kBuf;
    auto issue_k = [&]() {
#pragma unroll
        for (int kb = 0; kb < MB; ++kb) {
            if (kb < nlive) {
#pragma unroll
                for (int i = 0; i < kPP; ++i) {
                    const int piece = w * kPP + i;
                    int row, sw;
                    if (D == 128) {
                        row = piece * 8 + (l >> 3), sw = ((l & 7) ^ ((row >> 1) & 7)) << 4;
                    } else {
                        const int r16 = l >> 2;
                        row = piece * 16 + r16, sw = ((l & 3) ^ (((r16 >> 3) & 1) << 1)) << 4;
                    }
                    const int key = min(kb * kBlock + row, a.Sk - 1);
                    dma16(a.k8 + ((long)bh * a.Sk + key) * D + sw, k0 + kb * kBuf + piece * 1024);
                }
            }
        }
    };
    auto issue_v = [&]() {
#pragma unroll
        for (int kb = 0; kb < MB; ++kb) {
            if (kb < nlive) {
#pragma unroll
                for (int i = 0; i < kPP; ++i) {
                    const int piece = w * kPP + i, vrow = piece * 8 + (l >> 3), sw = ((l & 7) ^ ((vrow >> 1) & 7)) << 4;
                    dma16(a.vt8 + ((long)bh * D + vrow) * skp + kb * kBlock + sw, v0 + kb * kBuf + piece * 1024);
                }
            }
        }
    };
    issue_k();
    if (!kShare<D, MB>) issue_v();
    const v8i qf = {(int)qlo.x, (int)qlo.y, (int)qlo.z, (int)qlo.w, (int)qhi.x, (int)qhi.y, (int)qhi.z, (int)qhi.w};
    const int f_lo = D == 128 ? chunk_off(r, g) : r * 64 + ((g ^ (((r >> 3) & 1) << 1)) << 4), f_hi = chunk_off(r, 4 + g);
    const int f_v0 = chunk_off(r, g), f_v1 = chunk_off(r, 4 + g);          // V^T: tiles 0-3 and 4-7 of the block are one 16-byte chunk each
    // how many of the four tiles of half c of block kb does one of this wave's rows reach?  (wmax <= Sk: none beyond the last key)
    auto tiles_of = [&](int kb, int c) { return min(4, max(0, (wmax - (kb * kBlock + 64 * c) + 15) >> 4)); };

    float e[MB][8][4];                                                     // this wave's strip: logits, then their exponentials
    float mx = -INFINITY;
    // ---- sweep 1: scores.  K is here when all but the V^T requests have arrived
    if (kShare<D, MB>) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else wait_dma_but_blocks<kPP>(nlive);
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int kb = 0; kb < MB; ++kb) {
        if (kb < nlive) {
            const uint8_t *blk = lds + kb * kBuf;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int key0 = kb * kBlock + 64 * c, nt = tiles_of(kb, c);
                const int left = a.Sk - key0 - 4 * g;                      // this lane's columns j * 16 + e >= left do not exist
                const bool tail = key0 + 64 > a.Sk;
                float (*ev)[4] = &e[kb][4 * c];
                if (nt == 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) ev[j][0] = ev[j][1] = ev[j][2] = ev[j][3] = -INFINITY;
                } else if (full) {
                    score_half<F, D, 6>(blk, 4 * c, qf, f_lo, f_hi, a.scaling, ev, mx, mrow, key0, 0, tail ? nt : 4, left);
                } else if (!simple || key0 + 64 <= wmin) {
                    if (tail) score_half<F, D, 4>(blk, 4 * c, qf, f_lo, f_hi, a.scaling, ev, mx, nullptr, key0, 0, nt, left);
                    else score_half<F, D, 0>(blk, 4 * c, qf, f_lo, f_hi, a.scaling, ev, mx, nullptr, key0, 0, 4);
                } else {
                    if (tail) score_half<F, D, 5>(blk, 4 * c, qf, f_lo, f_hi, a.scaling, ev, mx, nullptr, key0 + 4 * g, my_live, nt, left);
                    else score_half<F, D, 1>(blk, 4 * c, qf, f_lo, f_hi, a.scaling, ev, mx, nullptr, key0 + 4 * g, my_live, nt);
                }
            }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (kShare<D, MB>) {                                                   // everyone is through sweep 1: the V^T blocks replace the K blocks
        __builtin_amdgcn_s_barrier();
        issue_v();
    }
    // ---- exponentials, once (a column at the bf16 minimum, beyond the extents or beyond Sk gives exactly 0)
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
                // staged as in the split kernel: half of the V^T fragments are requested before the codes are formed, the rest before the MFMAs
                const uint8_t *vblk = lds + (kShare<D, MB> ? 0 : nkb * kBuf) + kb * kBuf;
                u32x4 vlo[kDT], vhi[kDT];
#pragma unroll
                for (int dt = 0; dt < kDT / 2; ++dt) {
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
#pragma unroll
                for (int dt = kDT / 2; dt < kDT; ++dt) {
                    vlo[dt] = *(const u32x4 *)(vblk + dt * 2048 + f_v0);
                    vhi[dt] = *(const u32x4 *)(vblk + dt * 2048 + f_v1);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int dt = 0; dt < kDT; ++dt) {
                    const v8i vf = {(int)vlo[dt].x, (int)vlo[dt].y, (int)vlo[dt].z, (int)vlo[dt].w, (int)vhi[dt].x, (int)vhi[dt].y, (int)vhi[dt].z, (int)vhi[dt].w};
                    acc[dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf, acc[dt], F, F, 0, kUnit, 0, kUnit);
                }
            }
        }
    }
    // ---- the finished 64 x D tile leaves through LDS: every wave rounds its own 16 rows -- bf16 values when they are wanted, codes when
    // they are -- into the operand images, which are dead by now, and then the waves store 16 bytes a lane: whole rows of `out` / `out8`
    const int prow = w * 16 + r;
    uint8_t *tile_v = lds, *tile_c = lds + 64 * kValRow<D>;
    __syncthreads();                                                       // everyone is through sweep 2
    {
        uint8_t *vrow = tile_v + prow * kValRow<D> + 8 * g, *crow = tile_c + prow * kCodeRow<D> + 4 * g;          // this lane's columns 16 dt + 4 g ..
        const bool oe5 = a.out_fmt.p0 == 2;
#pragma unroll
        for (int j = 0; j < kDT; j += 2) {
            uint32_t o[4] = {pack_bf16x2(acc[j][0], acc[j][1]), pack_bf16x2(acc[j][2], acc[j][3]), pack_bf16x2(acc[j + 1][0], acc[j + 1][1]),
                             pack_bf16x2(acc[j + 1][2], acc[j + 1][3])};
            if (a.out8) {
                const uint2 codes = oe5 ? fq8_hw_vec8<true>(o, a.out_fmt) : fq8_hw_vec8<false>(o, a.out_fmt);
                *(uint32_t *)(crow + j * 16) = codes.x;
                *(uint32_t *)(crow + j * 16 + 16) = codes.y;
            }
            if (a.out) {
                *(uint2 *)(vrow + j * 32) = uint2{o[0], o[1]};
                *(uint2 *)(vrow + j * 32 + 32) = uint2{o[2], o[3]};
            }
        }
    }
    __syncthreads();
    const int rows = min(64, a.Sq - q0);                                   // rows >= Sq are never stored
    const long orow0 = ((long)b * a.Sq + q0) * a.H + h;                    // row q0 of this head, in rows of D elements; the next is H further
    if (a.out) {
        constexpr int kCh = D / 8;                                         // 16-byte chunks of a row of values
#pragma unroll
        for (int i = 0; i < 64 * kCh / 256; ++i) {
            const int c = t + i * 256, row = c / kCh, ch = c % kCh;
            if (row < rows) *(u32x4 *)((uint8_t *)a.out + (orow0 + (long)row * a.H) * (2 * D) + 16 * ch) = *(const u32x4 *)(tile_v + row * kValRow<D> + 16 * ch);
        }
    }
    if (a.out8) {
        constexpr int kCh = D / 16;                                        // 16-byte chunks of a row of codes
#pragma unroll
        for (int i = 0; i < 64 * kCh / 256; ++i) {
            const int c = t + i * 256, row = c / kCh, ch = c % kCh;
            if (row < rows) *(u32x4 *)(a.out8 + (orow0 + (long)row * a.H) * D + 16 * ch) = *(const u32x4 *)(tile_c + row * kCodeRow<D> + 16 * ch);
        }
    }
}

// fq_v(V) as FP8 codes, transposed to [d][slot] with rows of Skp = 128 ceil(Sk / 128) bytes, the slot <-> key permutation of
// qt_value_codes.h inside every 128-block, and code 0 in the slots of the keys >= Sk (which are not read).  One workgroup per
// (batch * head, key block).
template <bool E5M2, int D>
__global__ __launch_bounds__(256) void value_codes_t_ragged_kernel(const uint16_t *v, uint8_t *vt8, int H, long Sk, long sb, long sh, long sk, qt_format fmt) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[D * kBlock];
    const int t = threadIdx.x, kb = blockIdx.x;
    const long bh = blockIdx.y, b = bh / H, h = bh % H, skp = (Sk + kBlock - 1) / kBlock * kBlock;
#pragma unroll
    for (int it = 0; it < D / 16; ++it) {
        const int vi = it * 256 + t, key = vi / (D / 8), dv = vi % (D / 8);
        uint2 codes = {0u, 0u};
        if ((long)kb * kBlock + key < Sk) {
            const uint4 in = *(const uint4 *)(v + b * sb + h * sh + ((long)kb * kBlock + key) * sk + dv * 8);
            uint32_t o[4] = {in.x, in.y, in.z, in.w};
            codes = fq8_hw_vec8<E5M2>(o, fmt);
        }
        const int p = (key & 64) | (((key >> 2) & 3) << 4) | (((key >> 4) & 3) << 2) | (key & 3);
#pragma unroll
        for (int j = 0; j < 8; ++j) tile[(dv * 8 + j) * kBlock + p] = (uint8_t)((j < 4 ? codes.x >> (8 * j) : codes.y >> (8 * (j - 4))) & 0xFFu);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < D / 32; ++it) {
        const int ci = it * 256 + t, d = ci >> 3, ch = ci & 7;
        *(uint4 *)(vt8 + (bh * D + d) * skp + (long)kb * kBlock + ch * 16) = *(const uint4 *)(tile + d * kBlock + ch * 16);
    }
}

template <int F, int D, int MB>
int launch_ragged_mb(const AttnArgs &a, long BH, int nqb, int nkb, hipStream_t st) {
    static_assert(kBlock * D * (kShare<D, MB> ? 3 : 2) >= 64 * (kValRow<D> + kCodeRow<D>), "the finished tile reuses the operand images, at their smallest too");
    static_assert(MB * kBlock * D * (kShare<D, MB> ? 1 : 2) <= 64 * 1024, "no opt-in for the dynamic LDS needed");
    const int bytes = nkb * kBlock * D * (kShare<D, MB> ? 1 : 2);
    attention_fp8_ragged_kernel<F, D, MB><<<dim3((unsigned)BH, (unsigned)nqb), 256, bytes, st>>>(a);
    return qt_launch_status();
}

template <int F, int D>
int launch_ragged(const AttnArgs &a, long BH, int nqb, hipStream_t st) {
    const int nkb = (a.Sk + kBlock - 1) / kBlock;
    if (nkb <= 1) return launch_ragged_mb<F, D, 1>(a, BH, nqb, nkb, st);
    if (nkb <= 2) return launch_ragged_mb<F, D, 2>(a, BH, nqb, nkb, st);
    return launch_ragged_mb<F, D, 4>(a, BH, nqb, nkb, st);
}

template <bool E5M2, int D>
void launch_value_ragged(const dim3 &grid, hipStream_t st, const uint16_t *v, uint8_t *vt8, int H, long Sk, long sb, long sh, long sk, const qt_format &fmt) {
    value_codes_t_ragged_kernel<E5M2, D><<<grid, 256, 0, st>>>(v, vt8, H, Sk, sb, sh, sk, fmt);
}

}  // namespace

extern "C" {

int qt_value_codes_t_ragged(const uint16_t *v_dev, uint8_t *vt8_dev, long B, long H, long Sk, int head_dim, long stride_b, long stride_h, long stride_k,
                            const qt_format *fmt, void *stream) {
    if (B * H * Sk == 0) return QT_OK;
    const int f8 = qt_fp8_code(fmt);
    if (!v_dev || !vt8_dev || B < 0 || H < 1 || Sk < 0 || B * H > 65535 || (head_dim != 64 && head_dim != 128) || !f8) return QT_ERR_BAD_ARG;
    if ((((uintptr_t)v_dev | (uintptr_t)vt8_dev) & 15u) || ((stride_b | stride_h | stride_k) & 7)) return QT_ERR_UNALIGNED;
    const dim3 grid((unsigned)((Sk + kBlock - 1) / kBlock), (unsigned)(B * H));
    hipStream_t st = (hipStream_t)stream;
    if (head_dim == 128) {
        if (f8 == 2) launch_value_ragged<true, 128>(grid, st, v_dev, vt8_dev, (int)H, Sk, stride_b, stride_h, stride_k, *fmt);
        else launch_value_ragged<false, 128>(grid, st, v_dev, vt8_dev, (int)H, Sk, stride_b, stride_h, stride_k, *fmt);
    } else {
        if (f8 == 2) launch_value_ragged<true, 64>(grid, st, v_dev, vt8_dev, (int)H, Sk, stride_b, stride_h, stride_k, *fmt);
        else launch_value_ragged<false, 64>(grid, st, v_dev, vt8_dev, (int)H, Sk, stride_b, stride_h, stride_k, *fmt);
    }
    return qt_launch_status();
}

int qt_attention_fp8_ragged(const uint8_t *q8_dev, const uint8_t *k8_dev, const uint8_t *vt8_dev, int operand_format, const uint16_t *mask_dev,
                            long mask_sb, long mask_sh, long mask_sq, const int *row_live_dev, long live_sb, long live_sh, long live_sq,
                            int mask_is_simple, const int *mask_irregular_dev, uint16_t *out_dev, uint8_t *out8_dev, const qt_format *out_format, long B,
                            int H, int Sq, int Sk, int head_dim, float scaling, void *stream) {
    if (B * H * Sq == 0) return QT_OK;
    if (!q8_dev || !k8_dev || !vt8_dev || (!out_dev && !out8_dev) || B < 0 || H < 1 || Sq < 1 || Sk < 1 || Sk > kBlock * kMaxBlocksRagged ||
        B * H > 65535 || operand_format < 0 || operand_format > 1 || (head_dim != 64 && head_dim != 128))
        return QT_ERR_BAD_ARG;
    if ((((uintptr_t)q8_dev | (uintptr_t)k8_dev | (uintptr_t)vt8_dev) & 15u) || ((uintptr_t)out_dev & 15u) || ((uintptr_t)mask_dev & 1u))
        return QT_ERR_UNALIGNED;                                           // (the mask: any element strides, any 2-byte-aligned base)
    if (out8_dev && !qt_fp8_code(out_format)) return QT_ERR_BAD_ARG;
    if ((uintptr_t)out8_dev & 15u) return QT_ERR_UNALIGNED;                 // both results leave in 16-byte stores
    AttnArgs a{q8_dev, k8_dev, vt8_dev, mask_dev, mask_sb, mask_sh, mask_sq, row_live_dev, live_sb, live_sh, live_sq, mask_is_simple ? 1 : 0,
               out_dev, H, Sq, Sk, scaling, out8_dev, out8_dev ? *out_format : qt_format{}, mask_irregular_dev};
    const int nqb = (Sq + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    if (head_dim == 128) return operand_format == 0 ? launch_ragged<0, 128>(a, B * H, nqb, st) : launch_ragged<1, 128>(a, B * H, nqb, st);
    return operand_format == 0 ? launch_ragged<0, 64>(a, B * H, nqb, st) : launch_ragged<1, 64>(a, B * H, nqb, st);
}

}  // extern "C"
