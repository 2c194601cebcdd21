// qt_attention_mxf.hip -- the attention core of the block-scaled FLOAT recipes in one launch, no prepare launch:
// Q.K^T, scaling, mask, softmax, the block quantizer of the probabilities and P.V, the B x H x S x S tensors never written.
//
// Replaces, in a converted graph whose two attention matmuls run as
//     fp8_e4m3 | fp8_e5m2 | fp4_e2m1 ,qs=microscaling,bs=32,ax=-1  x  the same ,ax=-2      (power-of-two scales)
// the span
//     matmul_mx(q, k^T)  ->  mul / div by a scalar  ->  + mask  ->  softmax(-1)  ->  quantize_mx(p, ax=-1)  ->  matmul_mx(p', v)
//                                                                    decomposed.py:304-363 (matmul_mx), 365-448 (quantize_mx)
// on the packed operands qt_quantize_mx_bf16 / qt_quantize_mx_strided_bf16 / qt_mx_pack already wrote for those matmuls, read in place:
// q codes [B H][Q][D bits / 8] + E8M0 [B H][Q][D / 32]; k codes [B H][C][D bits / 8] + E8M0 [B H][C][D / 32] (the SECOND layout of
// K^T quantized along axis -2); v codes [B H][D][C bits / 8] + E8M0 [B H][D][C / 32] (the SECOND layout of V: V^T).  bf16 graphs,
// block size 32, one element format for all four operands.
//
// Rounding chain -- that of the nodes the launch replaces:
//   1. scores   one v_mfma_scale_f32_16x16x128_f8f6f4 over head_dim (head_dim 64: zeros in the upper half, as qt_mx_gemm's k tile
//               holds them) from C = 0, the fp32 sum rounded to bf16;
//   2. scaling  bf16(t * c) or bf16(t / c), c in fp32 (t / c the correctly rounded quotient: csrc/qt_attention_mxi.hip says where
//               torch's device node differs);
//   3. mask     bf16(t + mask);
//   4. softmax  in fp32 on those bf16 logits over the whole row, p = bf16(exp2((t - max) log2e) / sum);
//   5. P's quantizer (quantize_mx_kernel, csrc/qt_mx_quant.hip), with the shared code of qt_mx.h: per (row, 32-key block) amax ->
//               qt_mx::block_scale<kIoBf16> (force_scale_power_of_two, the in-dtype floor_log2_dtype) -> the E8M0 byte; per element
//               map[bf16(p * 2^-e)] (p / s where 2^-e is no normal number) through P's own 65 536-entry value map -- the map, not a
//               closed form: fpN_eXmY maps carry thresholds of the reference's bf16 arithmetic in their subnormal range --, the
//               element codes by qt_mx::vec_codes, a flushed block (scale below 2^-127) all zero codes: the bytes
//               qt_quantize_mx_bf16 packs for that row of p;
//   6. P.V      the scaled instruction again, the 128-key stages accumulated in increasing key order through its C operand, as
//               qt_mx_gemm's k loop does;
//   7. one rounding to bf16.
// A row whose logits are all -inf is NaN (softmax's 0 / 0), and only that row.
//
// P's block scale needs the NORMALISED probability, so the keys are streamed twice (qt_attention_mxi.hip, qt_attention_fp8_long.hip):
//   sweep 1   K stages of 128 keys (codes and E8M0 bytes) through a ring of LDS stages; per stage the 8 score tiles, the running
//             maximum and sum, lane-local; the four partial sums of a row meet in two shuffles behind the last stage.
//   sweep 2   K and V^T stages through the same ring; the same score tiles again (same instruction, same operands: the same bits),
//             the probabilities, their block quantizer, P.V.
// A workgroup = 4 waves owns 64 query rows of one (b, h), a wave 16 of them against ALL keys: nothing but the ring passes through LDS
// and the only barriers are the ring's.  The operands are multiplied swapped, S^T = K.Q^T: the result lane (r, g) holds query r
// against A rows m = 4 g + i of each of the stage's 8 tiles t, and the A row m of tile t is read from the key row
//     fp4   32 (m / 4) + 4 t + (m % 4)                     fp8   64 (t / 4) + 16 (m / 4) + 4 (t % 4) + (m % 4)
// so that the lane's 32 probabilities, taken in (t, i) order, are exactly the keys the P.V instruction wants in that lane's B operand
// in natural order: fp4 lanes hold k = 32 g + [0, 32) of the 128-deep step, fp8 lanes k = 16 g + [0, 16) and 64 + 16 g + [0, 16)
// (csrc/qt_mx_tile.h).  The block amax is in-lane for fp4; an fp8 lane holds one half of two blocks (g / 2 and 2 + g / 2), the other
// halves in lane l ^ 16: one shuffle, and one more hands every lane group g the E8M0 byte of block g, which is the B-side scale operand.
// V^T's code rows are read as they lie (no permutation, no transposition of P), its E8M0 byte is the A-side scale.  The mask is read
// as 8-byte pieces (four consecutive keys).
// Requests are LDS-DMA: 16-byte pieces for the codes (dma16), 4-byte pieces for the scale bytes (K's 4 D bytes of a stage are one
// contiguous run, V^T's are D rows x 4 bytes).  LDS images, in 16-byte slots s = row * chunks + chunk, the XOR applied to the source
// address of the request: the key rows a 16-lane group reads are 16 a + b or 32 a + b (a, b = 0..3), so the chunk is swizzled with
// a (and b / 2 for 128-byte rows); fp4 at head_dim 64 has 32-byte rows, where a's high bit moves the row by 4 instead.  V^T rows
// are read in natural order: the swizzles of qt_mx_tile.h's Tile.  The stage R - 1 ahead is requested in mid-iteration, behind the
// last ordinary load of the stage (mask, value map), so that no wait of the compiler's meets a fresh request.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_formats.h"
#include "qt_mx.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kKeys = 128;                                // keys per ring stage = one k step of the P.V instruction
constexpr int kMaxKeys = 16384;

template <int F, int D>
struct Stage {
    static constexpr int kBits = F < 2 ? 8 : 4;
    static constexpr int kRowK = D * kBits / 8, kChK = kRowK / 16;          // a key's code row: bytes, 16-byte chunks
    static constexpr int kRowV = kKeys * kBits / 8, kChV = kRowV / 16;      // a V^T row's share of the stage
    static constexpr int kCodes = kKeys * kRowK;                            // = D * kRowV
    static constexpr int kK = 0, kV = kCodes, kKS = 2 * kCodes, kVS = kKS + 512, kBytes = kVS + 512;
    static constexpr int kPieces = kCodes / 1024 / 4;                       // 1 KiB request pieces per wave and operand
    static constexpr int kScalePieces = D / 64;                             // 256-byte pieces of K's and of V^T's scale bytes
    static constexpr int kRing = 3 * kBytes <= 80 * 1024 ? 3 : 2;           // two workgroups per CU in every instantiation
};

struct MxfAttnArgs {
    const uint8_t *q, *k, *v;
    const uint8_t *eq, *ek, *ev;
    const uint16_t *mask;
    long msb, msh, msq;
    const uint16_t *pmap;                                 // P's value map
    uint16_t *out;
    int H, Q, C;
    float scaling;
    int div;
    float quant_max;
    int qmax_exp;
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

// dma16's 4-byte sibling: lane l's dword lands at LDS byte dst + 4 l (dst wave-uniform); M0 is written in the statement that reads it
__device__ __forceinline__ void dma4(const void *src, uint32_t dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 1\n\tglobal_load_lds_dword %0, off" ::"v"(src), "s"(dst) : "memory");
}

// 16-byte slot of chunk `chunk` of key row `row` in a stage's K image (an involution on the slot index, so the request of slot s'
// fetches kslot(s' / chunks, s' % chunks))
template <int F, int D>
__device__ __forceinline__ int kslot(int row, int chunk) {
    constexpr int CH = Stage<F, D>::kChK;
    const int s = row * CH + chunk;
    if constexpr (CH == 8) return s ^ (((row >> 1) & 1) | (((row >> 4) & 3) << 1));
    else if constexpr (CH == 4) return s ^ ((0x78 >> (2 * ((row >> (F < 2 ? 4 : 5)) & 3))) & 3);
    else return s ^ (((row >> 6) & 1) << 3);
}
// ... of V^T row `row` (a d): Tile<F>::chunk_off of qt_mx_tile.h
template <int F, int D>
__device__ __forceinline__ int vslot(int row, int chunk) {
    constexpr int CH = Stage<F, D>::kChV;
    const int s = row * CH + chunk;
    if constexpr (CH == 8) return s ^ ((row >> 1) & 7);
    else return s ^ ((0x78 >> (2 * ((row >> 2) & 3))) & 3);
}

template <int F, int D>
__global__ __launch_bounds__(256, 2) void attention_mxf_kernel(MxfAttnArgs a) {
    using S = Stage<F, D>;
    constexpr int kBits = S::kBits, kP = S::kPieces, kSP = S::kScalePieces, kRing = S::kRing;
    constexpr int kNB = D / 32;                           // 32-blocks of head_dim
    constexpr int kDT = D / 16;                           // output tiles of 16 d
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = l & 15, g = l >> 4;
    const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
    const int nkb = a.C / kKeys;
    const int q0 = (int)blockIdx.y * 64;
    const int qrow = q0 + w * 16 + r, qc = min(qrow, a.Q - 1);      // rows >= Q re-read the last row and are never stored
    const uint32_t l0 = lds_addr(lds);
    const long vrow_bytes = (long)a.C * kBits / 8, erow = a.C / 32;

    // ---- request geometry: lane l of a piece lands at byte 16 l (4 l) of it, so it fetches what the swizzle puts there
    const uint8_t *kp[kP], *vp[kP];
#pragma unroll
    for (int i = 0; i < kP; ++i) {
        const int slot = (w * kP + i) * 64 + l;
        const int ks = kslot<F, D>(slot / S::kChK, slot % S::kChK), vs = vslot<F, D>(slot / S::kChV, slot % S::kChV);
        kp[i] = a.k + ((long)bh * a.C + ks / S::kChK) * S::kRowK + (ks % S::kChK) * 16;             // + kb * 128 * kRowK
        vp[i] = a.v + ((long)bh * D + vs / S::kChV) * vrow_bytes + (vs % S::kChV) * 16;             // + kb * kRowV
    }
    // scale bytes: piece j of K's by wave j, piece j of V^T's (rows 64 j + l) by wave 2 + j
    const bool has_ks = w < kSP, has_vs = w >= 2 && w - 2 < kSP;
    const uint8_t *ksp = a.ek + (long)bh * a.C * kNB + (w % 2) * 256 + 4 * l;                       // + kb * 128 * kNB
    const uint8_t *vsp = a.ev + ((long)bh * D + (w % 2) * 64 + l) * erow;                           // + kb * 4
    auto issue = [&](int kb, bool with_v) {                         // kb < nkb: inside every array
        const uint32_t dst = l0 + (kb % kRing) * S::kBytes;
#pragma unroll
        for (int i = 0; i < kP; ++i) dma16(kp[i] + (long)kb * kKeys * S::kRowK, dst + S::kK + (w * kP + i) * 1024);
        if (has_ks) dma4(ksp + (long)kb * kKeys * kNB, dst + S::kKS + (w % 2) * 256);
        if (with_v) {
#pragma unroll
            for (int i = 0; i < kP; ++i) dma16(vp[i] + (long)kb * S::kRowV, dst + S::kV + (w * kP + i) * 1024);
            if (has_vs) dma4(vsp + kb * 4, dst + S::kVS + (w % 2) * 256);
        }
    };
    const int per1 = kP + has_ks, per2 = 2 * kP + has_ks + has_vs;  // this wave's requests per stage
    // allowed to remain outstanding in front of stage kb: the stages requested behind it
    auto ahead = [&](int kb) { return min(kRing - 2, nkb - 1 - kb); };

    // ---- the query fragment (B operand of S^T) and its scale byte
    const uint8_t *qp = a.q + ((long)bh * a.Q + qc) * S::kRowK;
    v8i qf = {0, 0, 0, 0, 0, 0, 0, 0};
    if (S::kChK >= 4 || g < 2) {
        const v4i lo = *(const v4i *)(qp + 16 * g);
        qf[0] = lo[0]; qf[1] = lo[1]; qf[2] = lo[2]; qf[3] = lo[3];
    }
    if constexpr (S::kChK == 8) {
        const v4i hi = *(const v4i *)(qp + 64 + 16 * g);
        qf[4] = hi[0]; qf[5] = hi[1]; qf[6] = hi[2]; qf[7] = hi[3];
    }
    const int sq = g < kNB ? (int)a.eq[((long)bh * a.Q + qc) * kNB + g] : 127;
    // first key of the lane's four of tile tt, within the stage
    auto key0 = [&](int tt) { return F < 2 ? 64 * (tt >> 2) + 16 * g + 4 * (tt & 3) : 32 * g + 4 * tt; };
    const uint16_t *mrow = a.mask ? a.mask + b * a.msb + h * a.msh + (long)qc * a.msq : nullptr;
    wait_vm(0);                                                     // the compiler's waits for these must not meet the stage requests

    // the 32 logits of stage kb as bf16 values: lg[tt][i] = key 128 kb + key0(tt) + i
    auto stage_logits = [&](const uint8_t *st, int kb, float (&lg)[8][4]) {
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            const int key = F < 2 ? 64 * (tt >> 2) + 16 * (r >> 2) + 4 * (tt & 3) + (r & 3) : 32 * (r >> 2) + 4 * tt + (r & 3);
            v8i kf = {0, 0, 0, 0, 0, 0, 0, 0};
            v4i lo = *(const v4i *)(st + S::kK + 16 * kslot<F, D>(key, S::kChK >= 4 ? g : (g & 1)));
            if (S::kChK < 4 && g >= 2) lo = v4i{0, 0, 0, 0};
            kf[0] = lo[0]; kf[1] = lo[1]; kf[2] = lo[2]; kf[3] = lo[3];
            if constexpr (S::kChK == 8) {
                const v4i hi = *(const v4i *)(st + S::kK + 16 * kslot<F, D>(key, 4 + g));
                kf[4] = hi[0]; kf[5] = hi[1]; kf[6] = hi[2]; kf[7] = hi[3];
            }
            int sk = st[S::kKS + key * kNB + (g & (kNB - 1))];
            if (g >= kNB) sk = 127;
            const v4f s = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf, v4f{0.f, 0.f, 0.f, 0.f}, F, F, 0, sk, 0, sq);
            uint2 mk = {0u, 0u};
            if (mrow) mk = *(const uint2 *)(mrow + kb * kKeys + key0(tt));
            const float mv[4] = {bf_lo(mk.x), bf_hi(mk.x), bf_lo(mk.y), bf_hi(mk.y)};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = bf16_round(s[i]);
                v = a.div ? bf16_round(v / a.scaling) : bf16_round(v * a.scaling);
                if (mrow) v = bf16_round(v + mv[i]);
                lg[tt][i] = v;
            }
        }
    };

    const float kLog2e = 1.4426950408889634f;
    float lg[8][4];
    float m = -INFINITY, lsum = 0.0f;

    // ---- sweep 1: the row maximum and the sum of exponentials.  Stage kb lives in slot kb % R; stage kb + R - 1 is requested in
    // iteration kb, behind its barrier -- everyone is through stage kb - 1, that slot's last.
#pragma unroll
    for (int i = 0; i < kRing - 1; ++i)
        if (i < nkb) issue(i, false);
    for (int kb = 0; kb < nkb; ++kb) {
        wait_vm(ahead(kb) * per1);
        __builtin_amdgcn_s_barrier();
        stage_logits(lds + (kb % kRing) * S::kBytes, kb, lg);
        if (kb + kRing - 1 < nkb) issue(kb + kRing - 1, false);
        float bm = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) bm = fmaxf(fmaxf(fmaxf(bm, lg[tt][0]), fmaxf(lg[tt][1], lg[tt][2])), lg[tt][3]);
        bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float mn = fmaxf(m, bm);
        const float ref = mn == -INFINITY ? 0.0f : mn;              // only -inf logits so far: every term is 0, not inf - inf
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            s0 += __builtin_amdgcn_exp2f((lg[tt][0] - ref) * kLog2e);
            s1 += __builtin_amdgcn_exp2f((lg[tt][1] - ref) * kLog2e);
            s0 += __builtin_amdgcn_exp2f((lg[tt][2] - ref) * kLog2e);
            s1 += __builtin_amdgcn_exp2f((lg[tt][3] - ref) * kLog2e);
        }
        lsum = lsum * __builtin_amdgcn_exp2f((m - ref) * kLog2e) + (s0 + s1);
        m = mn;
    }
    __builtin_amdgcn_s_barrier();                                   // everyone is through sweep 1 (no request is outstanding)
#pragma unroll
    for (int i = 0; i < kRing - 1; ++i)
        if (i < nkb) issue(i, true);
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
        wait_vm(ahead(kb) * per2);
        __builtin_amdgcn_s_barrier();
        const uint8_t *st = lds + (kb % kRing) * S::kBytes;
        stage_logits(st, kb, lg);
        // probabilities as bf16 pairs, and the block amax on their bit patterns (not negative; NaN patterns win): fp4 -- the lane's 32
        // keys are one block; fp8 -- tiles 0-3 are half of block g / 2, tiles 4-7 half of block 2 + g / 2, the other halves in lane l ^ 16
        uint32_t pw[8][2], am[2] = {0u, 0u};
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            float p[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) p[i] = __builtin_amdgcn_exp2f((lg[tt][i] - mref) * kLog2e) * inv;
            pw[tt][0] = pack_bf16x2(p[0], p[1]);
            pw[tt][1] = pack_bf16x2(p[2], p[3]);
            am[tt >> 2] = pk_max_u16(am[tt >> 2], pk_max_u16(pw[tt][0] & 0x7FFF7FFFu, pw[tt][1] & 0x7FFF7FFFu));
        }
        qt_mx::BlockScale sc[2];
        if constexpr (F < 2) {
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
                uint32_t x = max(am[hb] & 0xFFFFu, am[hb] >> 16);
                x = max(x, (uint32_t)__shfl_xor((int)x, 16, 64));
                sc[hb] = qt_mx::block_scale<kIoBf16>(x << 16, true, a.quant_max, a.qmax_exp, nullptr);
            }
        } else {
            const uint32_t x = pk_max_u16(am[0], am[1]);
            sc[0] = sc[1] = qt_mx::block_scale<kIoBf16>(max(x & 0xFFFFu, x >> 16) << 16, true, a.quant_max, a.qmax_exp, nullptr);
        }
        // the element step of quantize_mx_kernel: map[bf16(p / s)], eight values to a vec_codes
        v8i pf = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const qt_mx::BlockScale &bs = sc[j >> 1];
            const bool recip_ok = bs.recip_ok();
            const float rcp = bs.recip(), s = bs.s;
            float qv[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t word = pw[2 * j + (e >> 1)][e & 1];
                const float x0 = bf_lo(word), x1 = bf_hi(word);
                const uint32_t qw = recip_ok ? pack_bf16x2(x0 * rcp, x1 * rcp) : pack_bf16x2(x0 / s, x1 / s);
                qv[2 * e] = qt_bf2f(a.pmap[qw & 0xFFFFu]);
                qv[2 * e + 1] = qt_bf2f(a.pmap[qw >> 16]);
            }
            qt_mx::VecCodes<kBits> vc = qt_mx::vec_codes<kBits>(qv, F);
            if (bs.flush()) vc.w[0] = vc.w[1] = 0u;
            if constexpr (F < 2) { pf[2 * j] = (int)vc.w[0]; pf[2 * j + 1] = (int)vc.w[1]; }
            else pf[j] = (int)vc.w[0];
        }
        // the B-side scale operand: lane group g carries the byte of block g
        int sp = sc[0].e8m0();
        if constexpr (F < 2) {
            const int both = __shfl((int)sc[0].e8m0() | ((int)sc[1].e8m0() << 8), r + 32 * (g & 1), 64);
            sp = (both >> (8 * (g >> 1))) & 0xFF;
        }
        asm volatile("" ::"v"(pf), "v"(sp));                       // the map's gathers are consumed in front of the request
        if (kb + kRing - 1 < nkb) issue(kb + kRing - 1, true);
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) {
            const int d = 16 * dt + r;
            v8i vf = {0, 0, 0, 0, 0, 0, 0, 0};
            const v4i lo = *(const v4i *)(st + S::kV + 16 * vslot<F, D>(d, g));
            vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
            if constexpr (F < 2) {
                const v4i hi = *(const v4i *)(st + S::kV + 16 * vslot<F, D>(d, 4 + g));
                vf[4] = hi[0]; vf[5] = hi[1]; vf[6] = hi[2]; vf[7] = hi[3];
            }
            const int sv = st[S::kVS + 4 * d + g];
            acc[dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf, acc[dt], F, F, 0, sv, 0, sp);
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

template <int F, int D>
int launch_mxf_attention(const MxfAttnArgs &a, long BH, hipStream_t st) {
    constexpr int kLds = Stage<F, D>::kRing * Stage<F, D>::kBytes;  // fp8: 66 KiB at head_dim 128, 51 KiB at 64; fp4: 51 and 27 KiB
    if (const int rc = qt_allow_lds<attention_mxf_kernel<F, D>>(kLds)) return rc;
    attention_mxf_kernel<F, D><<<dim3((unsigned)BH, (unsigned)((a.Q + 63) / 64)), 256, kLds, st>>>(a);
    return qt_launch_status();
}

template <int F>
int launch_mxf_format(const MxfAttnArgs &a, long BH, int head_dim, hipStream_t st) {
    return head_dim == 128 ? launch_mxf_attention<F, 128>(a, BH, st) : launch_mxf_attention<F, 64>(a, BH, st);
}

}  // namespace

extern "C" int qt_attention_mxf(const uint8_t *q_codes, const uint8_t *q_e8m0, const uint8_t *k_codes, const uint8_t *k_e8m0, const uint8_t *v_codes,
                                const uint8_t *v_e8m0, const uint16_t *mask_dev, long mask_sb, long mask_sh, long mask_sq, float scaling,
                                int scaling_is_div, int p_format, const uint16_t *p_map_dev, float quant_max, uint16_t *out_dev, long B, int H,
                                int Q, int C, int head_dim, int block_size, void *stream) {
    if (!q_codes || !q_e8m0 || !k_codes || !k_e8m0 || !v_codes || !v_e8m0 || !p_map_dev || !out_dev) return QT_ERR_BAD_ARG;
    if (B < 0 || H < 1 || Q < 0 || block_size != 32 || (head_dim != 64 && head_dim != 128) || C < kKeys || C % kKeys != 0 || C > kMaxKeys ||
        B * H > 65535 || (Q + 63) / 64 > 65535)
        return QT_ERR_BAD_ARG;
    if (p_format != QT_MX_E4M3 && p_format != QT_MX_E5M2 && p_format != QT_MX_E2M1) return QT_ERR_BAD_ARG;
    if (!(quant_max > 0.0f) || !(quant_max < INFINITY) || !(scaling == scaling) || (scaling_is_div != 0 && scaling_is_div != 1))
        return QT_ERR_BAD_ARG;
    if (B * H * Q == 0) return QT_OK;
    if ((((uintptr_t)q_codes | (uintptr_t)k_codes | (uintptr_t)v_codes) & 15u) || (((uintptr_t)k_e8m0 | (uintptr_t)v_e8m0) & 3u) ||
        ((uintptr_t)out_dev & 7u) || ((uintptr_t)p_map_dev & 1u) ||
        (mask_dev && (((uintptr_t)mask_dev & 7u) || ((mask_sb | mask_sh | mask_sq) & 3))))
        return QT_ERR_UNALIGNED;
    int qe = 0;
    (void)frexpf(quant_max, &qe);                                   // floor(log2(quant_max)) = qe - 1, as the quantize_mx launch derives it
    const MxfAttnArgs a{q_codes, k_codes, v_codes, q_e8m0, k_e8m0, v_e8m0, mask_dev, mask_sb, mask_sh, mask_sq, p_map_dev, out_dev, H, Q, C, scaling,
                        scaling_is_div, quant_max, qe - 1};
    hipStream_t st = (hipStream_t)stream;
    switch (p_format) {
        case QT_MX_E4M3: return launch_mxf_format<QT_MX_E4M3>(a, B * H, head_dim, st);
        case QT_MX_E5M2: return launch_mxf_format<QT_MX_E5M2>(a, B * H, head_dim, st);
        default: return launch_mxf_format<QT_MX_E2M1>(a, B * H, head_dim, st);
    }
}
