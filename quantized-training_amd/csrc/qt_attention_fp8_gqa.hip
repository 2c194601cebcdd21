// qt_attention_fp8_gqa.hip -- the streaming attention core on FP8 codes (qt_attention_fp8_long.hip) for GROUPED-QUERY heads: H query heads
// over Hkv = H / G key / value heads, G in {2, 4, 8} (Llama-3 / Mistral 32 over 8, TinyLlama 32 over 4, Llama-2-70B 64 over 8), K and V^T
// taken UNREPEATED -- k8 [B][Hkv][Sk][D], vt8 [B][Hkv][D][Sk] as qt_value_codes_t writes it with H = Hkv -- where the module chain
// (modules/quantizable/modeling_llama.py: repeat_kv before qk_matmul) multiplies G copies of both.  Query head h reads kv head h / G.
//
// A workgroup = 8 waves owns one (batch, kv head) and 128 query rows spread over the group's G query heads: R = 128 / G rows of each
// (64, 32, 16), so wave w = (8 / G) hg + wt owns rows q0 + 16 wt .. + 15 of query head G kvh + hg.  A wave walks ALL keys of every block
// for its 16 rows of ONE head, exactly as a wave of the streaming kernel does -- the same instructions on the same operands in the same
// order, so every row is bit for bit what qt_attention_fp8_long returns on K / V^T repeated G times -- and nothing meets in LDS but the
// rings.  The rings are the streaming kernel's (four K stages in sweep 1, two (K, V^T) stages in sweep 2, its swizzles), requested ONCE per
// workgroup by LDS-DMA, the 1 KiB pieces dealt over 8 waves: a block brought into LDS feeds 128 query rows instead of 64, and the G
// heads' requests for the same bytes are gone.  The mask, row_live and the device flag are addressed by QUERY head.  Under a row-extent
// mask a wave skips the tiles beyond its own 16 rows; the workgroup walks blocks up to the largest extent of any of its 128 rows (they
// differ between the heads only through the mask).  Row blocks heaviest first.  The finished tile leaves through the dead ring in
// (row, head, d) order: the G heads of a row are neighbours in out / out8, so a run of G D elements is contiguous.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_attention_fp8_core.h"

namespace {

constexpr int kMaxKeys = 16384;
constexpr int kStages1 = 4, kStages2 = 2;                                  // ring stages: K blocks in sweep 1, (K, V^T) pairs in sweep 2
constexpr int kRows = 128, kWaves = 8;                                     // (head, query row) pairs and waves of a workgroup

template <int N>
__device__ __forceinline__ void wait_dma() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// split_row_extents for a workgroup of G heads: nlive = key blocks holding an unmasked column of one of the 128 (head, row) pairs -- lane l
// looks at pairs l and l + 64, pair p = row p % R of head h0 + p / R --; wmax / wmin / my_live as there, over this wave's 16 rows of head h
__device__ __forceinline__ void gqa_row_extents(const AttnArgs &a, int b, int h0, int h, int q0, int qc, int l, int lgR, int nkb, int &nlive, int &wmax,
                                                int &wmin, int &my_live) {
    nlive = nkb, wmax = a.Sk, wmin = a.Sk, my_live = a.Sk;
    if (a.row_live) {
        int lv = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = l + 64 * i, qq = min(q0 + (p & ((1 << lgR) - 1)), a.Sq - 1);
            const int v = a.row_live[b * a.lsb + (h0 + (p >> lgR)) * a.lsh + qq * a.lsq];
            lv = max(lv, v <= 0 ? a.Sk : v);
        }
        my_live = a.row_live[b * a.lsb + h * a.lsh + qc * a.lsq];
        int hi = my_live <= 0 ? a.Sk : my_live, lo = max(my_live, 0);       // a fully masked row is walked to the end and masked from column 0
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) lv = max(lv, __shfl_xor(lv, off, 64));
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            hi = max(hi, __shfl_xor(hi, off, 64));
            lo = min(lo, __shfl_xor(lo, off, 64));
        }
        nlive = __builtin_amdgcn_readfirstlane(min(nkb, (lv + kBlock - 1) / kBlock));
        wmax = __builtin_amdgcn_readfirstlane(hi);
        wmin = __builtin_amdgcn_readfirstlane(lo);
    }
}

// F: operand format of q, k, v and p (0 = E4M3, 1 = E5M2); lgG = log2 G (1 .. 3) is a launch argument: it enters the index arithmetic of
// the prologue and of the stores only
template <int F, int D>
__global__ __launch_bounds__(512, 2) void attention_fp8_gqa_kernel(AttnArgs a, int Hkv, int lgG) {
    constexpr int kBuf = kBlock * D;                                       // one K / V^T block of codes: 16 KiB at head_dim 128, 8 KiB at 64
    constexpr int kPieces = D / 64;                                        // 1 KiB request pieces per wave and block: D / 8 over 8 waves
    constexpr int kDT = D / 16;                                            // output tiles of 16 d
    static_assert(kStages1 * kBuf == kStages2 * 2 * kBuf && kStages1 * kBuf <= 64 * 1024, "both rings fill the same 64 KiB at most");
    static_assert(kRows * (kValRow<D> + kCodeRow<D>) <= kStages1 * kBuf, "the finished tile reuses the ring");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = l & 15, g = l >> 4;
    const int lgR = 7 - lgG, R = 1 << lgR;                                 // query rows of each head in a workgroup
    const int bkv = blockIdx.x, b = bkv / Hkv, h0 = (bkv % Hkv) << lgG;    // the group's first query head
    const int hg = w >> (3 - lgG), wt = w & ((kWaves >> lgG) - 1), h = h0 + hg;
    const int nkb = a.Sk / kBlock, nqb = (a.Sq + R - 1) >> lgR;
    const int qb = nqb - 1 - (int)blockIdx.y;                              // the heaviest blocks of rows first under a causal mask
    const int q0 = qb << lgR;
    const int qrow = q0 + wt * 16 + r, qc = min(qrow, a.Sq - 1);
    int nlive, wmax, wmin, my_live;
    gqa_row_extents(a, b, h0, h, q0, qc, l, lgR, nkb, nlive, wmax, wmin, my_live);
    const bool simple = a.mask && a.row_live && (a.mask_simple || (a.mask_irregular && *a.mask_irregular == 0)), full = a.mask && !simple;
    if (!simple) wmin = a.Sk;                                              // extents then only bound the walk; inside them the mask is read
    if (!simple && !a.row_live) wmax = a.Sk;
    const uint32_t l0 = lds_addr(lds);
    // DMA: a block is D / 8 pieces of 1 KiB, this wave's are kPieces w ...; the pieces and their swizzles are the streaming kernel's
    // (K, head_dim 128: 8 key rows x 128 bytes, 16-byte chunks XOR-swizzled by the row; head_dim 64: 16 key rows x 64 bytes, chunk c of
    // row r in slot c ^ 2 (r >> 3 & 1); V^T: 8 rows (d) x 128 bytes (keys), the swizzle of the 128-byte K rows)
    const uint8_t *kp[kPieces], *vp[kPieces];
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
        const int piece = w * kPieces + i;
        if (D == 128) {
            const int row = piece * 8 + (l >> 3), slot = l & 7, sw = ((slot ^ ((row >> 1) & 7)) << 4);
            kp[i] = a.k8 + ((long)bkv * a.Sk + row) * D + sw;               // + block * 128 * D
        } else {
            const int r16 = l >> 2, row = piece * 16 + r16, sw = (((l & 3) ^ (((r16 >> 3) & 1) << 1)) << 4);
            kp[i] = a.k8 + ((long)bkv * a.Sk + row) * D + sw;
        }
        const int vrow = piece * 8 + (l >> 3), vslot = l & 7, vsw = ((vslot ^ ((vrow >> 1) & 7)) << 4);
        vp[i] = a.vt8 + ((long)bkv * D + vrow) * a.Sk + vsw;                // + block * 128
    }
    auto issue_k = [&](int kb, uint32_t dst) {                             // kb < nlive <= nkb: inside k8
#pragma unroll
        for (int i = 0; i < kPieces; ++i) dma16(kp[i] + (long)kb * kBuf, dst + (w * kPieces + i) * 1024);
    };
    auto issue_v = [&](int kb, uint32_t dst) {
#pragma unroll
        for (int i = 0; i < kPieces; ++i) dma16(vp[i] + (long)kb * kBlock, dst + (w * kPieces + i) * 1024);
    };
    const uint8_t *qp = a.q8 + (((long)b * a.H + h) * a.Sq + qc) * D;
    const u32x4 qlo = *(const u32x4 *)(qp + 16 * g), qhi = D == 128 ? *(const u32x4 *)(qp + 64 + 16 * g) : u32x4{0u, 0u, 0u, 0u};
    const uint16_t *mrow = full ? a.mask + b * a.msb + h * a.msh + (long)qc * a.msq + 4 * g : nullptr;
    wait_dma<0>();                                                         // the compiler's waits for these must not meet the block requests
    const v8i qf = {(int)qlo.x, (int)qlo.y, (int)qlo.z, (int)qlo.w, (int)qhi.x, (int)qhi.y, (int)qhi.z, (int)qhi.w};
    const int f_lo = D == 128 ? chunk_off(r, g) : r * 64 + ((g ^ (((r >> 3) & 1) << 1)) << 4), f_hi = chunk_off(r, 4 + g);
    const int f_v0 = chunk_off(r, g), f_v1 = chunk_off(r, 4 + g);          // V^T: tiles 0-3 and 4-7 of the block are one 16-byte chunk each
    // how many of block kb's 8 tiles does one of this wave's rows reach?
    auto tiles_of = [&](int kb) { return min(8, max(0, (wmax - kb * kBlock + 15) >> 4)); };
    // the 32 scores of block kb (nt = tiles_of(kb) > 0), in both sweeps: tiles beyond the wave's rows hold -inf (probability exactly 0)
    auto block_scores = [&](const uint8_t *blk, int kb, int nt, float (*ev)[4], float &mx) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int key0 = kb * kBlock + 64 * c, nth = min(4, nt - 4 * c);
            if (nth <= 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) ev[4 * c + j][0] = ev[4 * c + j][1] = ev[4 * c + j][2] = ev[4 * c + j][3] = -INFINITY;
            } else if (full) {
                score_half<F, D, 2>(blk, 4 * c, qf, f_lo, f_hi, a.scaling, ev + 4 * c, mx, mrow, key0, 0, 4);
            } else if (!simple || key0 + 64 <= wmin) {
                score_half<F, D, 0>(blk, 4 * c, qf, f_lo, f_hi, a.scaling, ev + 4 * c, mx, nullptr, key0, 0, 4);
            } else {
                score_half<F, D, 1>(blk, 4 * c, qf, f_lo, f_hi, a.scaling, ev + 4 * c, mx, nullptr, key0 + 4 * g, my_live, nth);
            }
        }
    };
    const float kLog2e = 1.4426950408889634f;
    float ev[8][4];
    float m = -INFINITY, lsum = 0.0f;

    // ---- sweep 1: the row maximum and the sum of exponentials.  Requests run three blocks ahead of the arithmetic; block kb lives in
    // stage kb % 4 and is requested behind the barrier of iteration kb - 3, when all 8 waves are through block kb - 4, the stage's last.
#pragma unroll
    for (int i = 0; i < kStages1 - 1; ++i)
        if (i < nlive) issue_k(i, l0 + i * kBuf);
    for (int kb = 0; kb < nlive; ++kb) {
        const int ahead = min(nlive - 1 - kb, kStages1 - 2);               // later blocks this wave has requested already
        if (ahead == 2) wait_dma<2 * kPieces>();
        else if (ahead == 1) wait_dma<kPieces>();
        else wait_dma<0>();
        __builtin_amdgcn_s_barrier();                                      // block kb is here; everyone is through block kb - 1
        if (kb + kStages1 - 1 < nlive) issue_k(kb + kStages1 - 1, l0 + ((kb + kStages1 - 1) % kStages1) * kBuf);
        const int nt = tiles_of(kb);
        if (nt == 0) continue;                                             // beyond every row of this wave: exactly 0 each
        float bm = -INFINITY;
        block_scores(lds + (kb % kStages1) * kBuf, kb, nt, ev, bm);
        bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float mn = fmaxf(m, bm);
        const float ref = mn == -INFINITY ? 0.0f : mn;                     // (only -inf logits so far: every term is 0, not inf - inf)
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (4 * (j >> 2) < nt) {
                s0 += __builtin_amdgcn_exp2f((ev[j][0] - ref) * kLog2e);
                s1 += __builtin_amdgcn_exp2f((ev[j][1] - ref) * kLog2e);
                s0 += __builtin_amdgcn_exp2f((ev[j][2] - ref) * kLog2e);
                s1 += __builtin_amdgcn_exp2f((ev[j][3] - ref) * kLog2e);
            }
        }
        lsum = lsum * __builtin_amdgcn_exp2f((m - ref) * kLog2e) + (s0 + s1);
        m = mn;
    }
    // everyone is through sweep 1: the first (K, V^T) pair is requested while the partial sums meet
    __builtin_amdgcn_s_barrier();
    issue_k(0, l0);
    issue_v(0, l0 + kBuf);
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = 1.0f / lsum;

    // ---- sweep 2: the same scores, the probabilities, P.V.  Block kb lives in stage kb % 2; the next pair is requested behind the barrier
    // that ends the arithmetic on the stage it replaces.
    v4f acc[kDT];
#pragma unroll
    for (int i = 0; i < kDT; ++i) acc[i] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nlive; ++kb) {
        wait_dma<0>();
        __builtin_amdgcn_s_barrier();
        if (kb + 1 < nlive) {
            const uint32_t dst = l0 + ((kb + 1) % kStages2) * (2 * kBuf);
            issue_k(kb + 1, dst);
            issue_v(kb + 1, dst + kBuf);
        }
        const int nt = tiles_of(kb);
        if (nt == 0) continue;
        const uint8_t *blk = lds + (kb % kStages2) * (2 * kBuf), *vblk = blk + kBuf;
        float unused = -INFINITY;
        block_scores(blk, kb, nt, ev, unused);
        // half of the V^T fragments are requested before the codes are formed, the rest before the MFMAs
        u32x4 vlo[kDT], vhi[kDT];
#pragma unroll
        for (int dt = 0; dt < kDT / 2; ++dt) {
            vlo[dt] = *(const u32x4 *)(vblk + dt * 2048 + f_v0);
            vhi[dt] = *(const u32x4 *)(vblk + dt * 2048 + f_v1);
        }
        uint32_t pd[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (4 * (j >> 2) < nt) {
                const float p0 = __builtin_amdgcn_exp2f((ev[j][0] - m) * kLog2e) * inv, p1 = __builtin_amdgcn_exp2f((ev[j][1] - m) * kLog2e) * inv;
                const float p2 = __builtin_amdgcn_exp2f((ev[j][2] - m) * kLog2e) * inv, p3 = __builtin_amdgcn_exp2f((ev[j][3] - m) * kLog2e) * inv;
                pd[j] = prob_codes<F == 1>(pack_bf16x2(p0, p1), pack_bf16x2(p2, p3));          // probabilities, bf16; fq_p
            } else {
                pd[j] = 0;
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
    // ---- the finished 128 x D tile leaves through LDS: every wave rounds its own 16 rows -- bf16 values when they are wanted, codes when
    // they are -- into the ring, which is dead by now (pair w 16 + r = hg R + 16 wt + r), and then all eight waves store 16 bytes a lane
    const int prow = w * 16 + r;
    uint8_t *tile_v = lds, *tile_c = lds + kRows * kValRow<D>;
    __syncthreads();                                                       // everyone is through sweep 2
    {
        uint8_t *vrow = tile_v + prow * kValRow<D> + 8 * g, *crow = tile_c + prow * kCodeRow<D> + 4 * g;     // this lane's columns 16 dt + 4 g ..
        if (a.out8) {
            const bool oe5 = a.out_fmt.p0 == 2;
#pragma unroll
            for (int j = 0; j < kDT; j += 2) {
                uint32_t o[4] = {pack_bf16x2(acc[j][0], acc[j][1]), pack_bf16x2(acc[j][2], acc[j][3]),
                                 pack_bf16x2(acc[j + 1][0], acc[j + 1][1]), pack_bf16x2(acc[j + 1][2], acc[j + 1][3])};
                const uint2 codes = oe5 ? fq8_hw_vec8<true>(o, a.out_fmt) : fq8_hw_vec8<false>(o, a.out_fmt);
                if (a.out) {
                    *(uint2 *)(vrow + j * 32) = uint2{o[0], o[1]};
                    *(uint2 *)(vrow + j * 32 + 32) = uint2{o[2], o[3]};
                }
                *(uint32_t *)(crow + j * 16) = codes.x;
                *(uint32_t *)(crow + j * 16 + 16) = codes.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kDT; ++j)
                *(uint2 *)(vrow + j * 32) = uint2{pack_bf16x2(acc[j][0], acc[j][1]), pack_bf16x2(acc[j][2], acc[j][3])};
        }
    }
    __syncthreads();
    // chunk c = (row, head of the group, 16-byte piece): the G heads of a query row are neighbours in [B][Sq][H][D], so consecutive lanes
    // write G D contiguous elements; rows >= Sq are never stored
    const int rows = min(R, a.Sq - q0);
    const long orow0 = ((long)b * a.Sq + q0) * a.H + h0;                   // row q0 of head h0, in rows of D elements; the next row is H further
    if (a.out) {
        constexpr int kCh = D / 8;                                         // 16-byte chunks of a row of values
#pragma unroll
        for (int i = 0; i < kRows * kCh / 512; ++i) {
            const int c = t + i * 512, ch = c % kCh, hh = (c / kCh) & ((1 << lgG) - 1), row = (c / kCh) >> lgG;
            if (row < rows)
                *(u32x4 *)((uint8_t *)a.out + (orow0 + (long)row * a.H + hh) * (2 * D) + 16 * ch) = *(const u32x4 *)(tile_v + ((hh << lgR) + row) * kValRow<D> + 16 * ch);
        }
    }
    if (a.out8) {
        constexpr int kCh = D / 16;                                        // 16-byte chunks of a row of codes
#pragma unroll
        for (int i = 0; i < kRows * kCh / 512; ++i) {
            const int c = t + i * 512, ch = c % kCh, hh = (c / kCh) & ((1 << lgG) - 1), row = (c / kCh) >> lgG;
            if (row < rows)
                *(u32x4 *)(a.out8 + (orow0 + (long)row * a.H + hh) * D + 16 * ch) = *(const u32x4 *)(tile_c + ((hh << lgR) + row) * kCodeRow<D> + 16 * ch);
        }
    }
}

template <int F, int D>
int launch_gqa(const AttnArgs &a, long BHkv, int Hkv, int lgG, int nqb, hipStream_t st) {
    constexpr int kLds = kStages1 * kBlock * D;                          // the ring: 64 KiB at head_dim 128, 32 KiB at 64
    if (qt_allow_lds<attention_fp8_gqa_kernel<F, D>>(kLds)) return QT_ERR_BAD_ARG;
    attention_fp8_gqa_kernel<F, D><<<dim3((unsigned)BHkv, (unsigned)nqb), 512, kLds, st>>>(a, Hkv, lgG);
    return qt_launch_status();
}

}  // namespace

extern "C" int qt_attention_fp8_gqa(const uint8_t *q8_dev, const uint8_t *k8_dev, const uint8_t *vt8_dev, int operand_format, const uint16_t *mask_dev,
                                    long mask_sb, long mask_sh, long mask_sq, const int *row_live_dev, long live_sb, long live_sh, long live_sq,
                                    int mask_is_simple, const int *mask_irregular_dev, uint16_t *out_dev, uint8_t *out8_dev, const qt_format *out_format,
                                    long B, int H, int Hkv, int Sq, int Sk, int head_dim, float scaling, void *stream) {
    if (!q8_dev || !k8_dev || !vt8_dev || (!out_dev && !out8_dev) || B < 0 || H < 1 || Hkv < 1 || H % Hkv != 0 || Sq < 0 || Sk < kBlock ||
        Sk % kBlock != 0 || Sk > kMaxKeys || B * Hkv > 65535 || operand_format < 0 || operand_format > 1 || (head_dim != 64 && head_dim != 128))
        return QT_ERR_BAD_ARG;
    const int G = H / Hkv, lgG = G == 2 ? 1 : G == 4 ? 2 : G == 8 ? 3 : 0;
    if (!lgG) return QT_ERR_BAD_ARG;                                        // G = 1: the entry points above; G = 3, 5, 6, 7, ...: nobody's
    if ((((uintptr_t)q8_dev | (uintptr_t)k8_dev | (uintptr_t)vt8_dev) & 15u) || ((uintptr_t)out_dev & 15u) ||
        (mask_dev && ((((uintptr_t)mask_dev) & 7u) || ((mask_sb | mask_sh | mask_sq) & 3))))
        return QT_ERR_UNALIGNED;
    if (out8_dev && !qt_fp8_code(out_format)) return QT_ERR_BAD_ARG;
    if ((uintptr_t)out8_dev & 15u) return QT_ERR_UNALIGNED;                 // both results leave in 16-byte stores
    const long nqb = ((long)Sq + (kRows >> lgG) - 1) >> (7 - lgG);
    if (nqb > 65535) return QT_ERR_BAD_ARG;
    if (B * Sq == 0) return QT_OK;
    AttnArgs a{q8_dev, k8_dev, vt8_dev, mask_dev, mask_sb, mask_sh, mask_sq, row_live_dev, live_sb, live_sh, live_sq, mask_is_simple ? 1 : 0,
               out_dev, H, Sq, Sk, scaling, out8_dev, out8_dev ? *out_format : qt_format{}, mask_irregular_dev};
    hipStream_t st = (hipStream_t)stream;
    if (head_dim == 128) return operand_format == 0 ? launch_gqa<0, 128>(a, B * Hkv, Hkv, lgG, (int)nqb, st) : launch_gqa<1, 128>(a, B * Hkv, Hkv, lgG, (int)nqb, st);
    return operand_format == 0 ? launch_gqa<0, 64>(a, B * Hkv, Hkv, lgG, (int)nqb, st) : launch_gqa<1, 64>(a, B * Hkv, Hkv, lgG, (int)nqb, st);
}
