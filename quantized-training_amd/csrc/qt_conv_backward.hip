// qt_conv_backward.hip -- the two backward products of a QAT Conv2d as implicit GEMMs on the matrix cores, in-tree.
//
// The reference's QAT Conv2d is self._conv_forward(input, self.weight_fake_quant(self.weight), self.bias) under autograd
// (modules/qat/conv.py:43-44; ConvBn2d: conv_fused.py:103-126): its backward is the library's convolution_backward on the incoming
// gradient, the saved input and the fake-quantized weight.  Both arrive here as bf16 VALUES; nothing here quantizes.
//     dgrad   gx[n, hi, wi, c]  = sum over (r, s, co) of gy[n, ho, wo, co] . wq[co, r, s, c]     hi + ph - r dh = ho sh,  wi + pw - s dw = wo sw
//     wgrad   gw[co, r, s, c]   = sum over m = (n, ho, wo) of gy[m, co] . x[n, ho sh - ph + r dh, wo sw - pw + s dw, c]
// NHWC activations and gradients, [Cout][kh][kw][Cin] weights and weight gradients (the forward's layouts, qt_conv.hip), fp32 accumulation
// on v_mfma_f32_16x16x32_bf16, ONE rounding to bf16, groups = 1, zero padding.  The order of an element's additions is fixed by the tile
// walk and, with split-K, by the split order: the same bits on every launch.
//
// dgrad as a GEMM.  Rows = the N H W input pixels, columns = Cin, K = kh kw Cout walked in k tiles of 64 output channels of ONE tap.  The A
// operand is gathered like the forward's: row m of k tile (r, s, co0) is the 128 contiguous bytes gy[n, ho, wo, co0 : co0 + 64] of the
// output pixel whose window holds input pixel m under tap (r, s).  There is none when the tap leaves the plane or the stride does not
// divide (ho = (hi + ph - r dh) / sh must be an integer in [0, Ho)); such lanes, rows past M and the tiles that pad a short contraction up
// to the ring's depth fetch a block of zeros -- a select, no branch in the k step.  Cout ragged against the k tile is declined.
// A lane keeps quotient and remainder of (hi + ph - r dh) / sh and of the column's: a tap step subtracts dh (dw) from them with one borrow,
// no division in the k loop.  The B operand is wq as it lies in memory: k rows co are kh kw Cin elements apart at the tap's offset, Cin
// contiguous -- the trans_b layout of qt_train_gemm.hip, staged [64 k][BN] and read through ds_read_b64_tr_b16.  Every element of gx is
// written, whether a tap reaches its pixel or not.
//
// wgrad as a GEMM.  Rows = Cout, columns = (r, s, c), K = the M = N Ho Wo output pixels in k tiles of 64 pixels.  Both operands have the
// contraction index as their row index ([64 k][columns] images, ds_read_b64_tr_b16): A is gy [M][Cout] as it stands, B is the forward's
// gathered activation -- a lane's 16 bytes are 8 channels of ONE tap (a column tile may span taps: the tap is the lane's, fixed over the
// k loop) of the input pixel its k row's output pixel reads, or zeros in the padding and past M.  A lane's (n, ho, wo) moves on by 64
// pixels per k tile with two carries.  The output is small and K is huge, so the contraction is split: `ksplit` workgroups share an
// output tile, each multiplies a contiguous range of k tiles and leaves its fp32 partial sums in the caller's workspace; the workgroup
// that draws the tile's last ticket adds them IN SPLIT ORDER, rounds once, and resets the ticket (the hand-off of qt_linear_fqt.hip:
// write-through stores, drained in front of the barrier that precedes the relaxed ticket; the owner reads past its L1).  The split
// factor is a fixed function of the shape and the CU count.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_gemm_ring.h"

namespace {

__device__ __attribute__((aligned(128))) const uint32_t kZeroRow[32] = {0};      // what dead lanes fetch

struct BwdArgs {
    const uint16_t *gy, *w, *x;
    uint16_t *out;                    // gx (dgrad) or gw (wgrad)
    float *ws;                        // wgrad, ksplit > 1: [tile][split][wave][fragment][64 lanes][4] fp32
    unsigned int *tickets;            // wgrad, ksplit > 1: [tile] arrival counters, zero between launches
    int N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, dh, dw;
    int Ho, Wo, M, Min;               // M = N Ho Wo output pixels, Min = N H W input pixels
    int tiles_m, tiles_n;
    int ksplit, kper, nkt;            // wgrad: splits, k tiles per split, k tiles in all
};

__device__ __forceinline__ void store16_sc1(const float *sbase, uint32_t voff, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, %2 sc1" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ f32x4 load16_sc1(const float *sbase, uint32_t voff) {
    f32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, %2 sc1" : "=v"(v) : "v"(voff), "s"(sbase) : "memory");
    return v;
}

// ---- dgrad ------------------------------------------------------------------------------------------------------------------------------
template <int BM, int BN>
__global__ __launch_bounds__(kThreads) void conv2d_dgrad_kernel(const BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int kAImg = BM * kBK * 2;
    constexpr int kStage = Ring<BM, BN>::kStage, S = Ring<BM, BN>::kStages;
    constexpr int kAV = BM / 64, kBV = BN / 64;
    constexpr int kPieces = kAV + kBV;
    constexpr int WM = BM / 64, WN = BN / 32;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), wr = wave >> 1, wc = wave & 1;
    const int total = a.tiles_m * a.tiles_n;
    const int tile = (a.tiles_m & 7) ? xcd_run((int)blockIdx.x, total) : (int)blockIdx.x;
    const int tn = tile / a.tiles_m, tm = tile % a.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kc = a.Cout / kBK;                                        // k tiles per tap (Cout % 64 == 0: the entry point declines the rest)
    const int nk_real = a.kh * a.kw * kc;
    const int nk = nk_real > S - 1 ? nk_real : S - 1;

    // ---- the address generator.  Per lane and gradient piece: (hi + ph) / sh and (wi + pw) / sw with their remainders -- tap (0, 0) --,
    // and the image's base address (+ the swizzled chunk); rows past M get a quotient no tap brings back.
    const unsigned char *pa[kAV], *sb[kBV];
    int qh[kAV], rh[kAV], qw[kAV], rw[kAV], qw0[kAV], rw0[kAV];
    uint32_t da[kAV], db[kBV];
    const unsigned char *zero = (const unsigned char *)kZeroRow + (lane & 7) * 16;
#pragma unroll
    for (int v = 0; v < kAV; ++v) {
        const int piece = v * 8 + wave;
        da[v] = piece * 1024;
        const int row = piece * 8 + (lane >> 3), pos = lane & 7, ch = pos ^ ((row >> 1) & 7);
        const int m = m0 + row, live = m < a.Min;
        const int mm = live ? m : 0;
        const int n = mm / (a.H * a.W), rem = mm - n * (a.H * a.W), hi = rem / a.W, wi = rem - hi * a.W;
        const int th = hi + a.ph, tw = wi + a.pw;
        qh[v] = th / a.sh; rh[v] = th - qh[v] * a.sh;
        qw0[v] = tw / a.sw; rw0[v] = tw - qw0[v] * a.sw;
        if (!live) qh[v] = -(1 << 28);
        qw[v] = qw0[v]; rw[v] = rw0[v];
        pa[v] = (const unsigned char *)(a.gy + (long)n * a.Ho * a.Wo * a.Cout) + ch * 16;
    }
    const long ldb = (long)a.kh * a.kw * a.Cin;                          // elements between two k rows of the weight
#pragma unroll
    for (int v = 0; v < kBV; ++v) {
        const int piece = v * 8 + wave;
        db[v] = kAImg + piece * 1024;
        constexpr int RB = BN * 2, kPos = RB / 16;
        const int row = (piece * 64 + lane) / kPos, pos = (piece * 64 + lane) % kPos;
        const int ch = (((pos >> 1) ^ s_tr<RB>(row)) << 1) | (pos & 1);
        sb[v] = (const unsigned char *)(a.w + (long)row * ldb + min(n0 + ch * 8, a.Cin - 8));
    }
    // what a tap step subtracts from a lane's quotient and remainder (dh = dhq sh + dhr)
    const int dhq = a.dh / a.sh, dhr = a.dh - dhq * a.sh, dwq = a.dw / a.sw, dwr = a.dw - dwq * a.sw;
    const long step_b = kBK * ldb * 2, next_tap_b = (long)a.Cin * 2 - (long)kc * step_b;
    const uint32_t l0 = lds_addr(lds);
    int rq_stage = 0;
    int tap_r = 0, tap_s = 0, tap_c = 0;                                // the k tile the next request fetches (wave-uniform)
    auto request = [&]() __attribute__((always_inline)) {
        const uint32_t st = l0 + rq_stage * kStage;
        const bool tile_ok = tap_r < a.kh;
        const bool wrap_c = tap_c + kBK == a.Cout;
        const bool wrap_s = wrap_c & (tap_s + 1 == a.kw);
#pragma unroll
        for (int v = 0; v < kAV; ++v) {
            const bool ok = tile_ok & ((rh[v] | rw[v]) == 0) & ((unsigned)qh[v] < (unsigned)a.Ho) & ((unsigned)qw[v] < (unsigned)a.Wo);
            const unsigned pix = (unsigned)qh[v] * (unsigned)a.Wo + (unsigned)qw[v];
            const unsigned char *px = pa[v] + ((unsigned long)pix * (unsigned)a.Cout + (unsigned)tap_c) * 2;
            dma16(ok ? px : zero, st + da[v]);
            // the next k tile's tap: column quotient one dw further (or back to tap column 0 and the row quotient one dh further)
            int nqw = qw[v] - dwq, nrw = rw[v] - dwr;
            nqw -= nrw < 0; nrw += nrw < 0 ? a.sw : 0;
            int nqh = qh[v] - dhq, nrh = rh[v] - dhr;
            nqh -= nrh < 0; nrh += nrh < 0 ? a.sh : 0;
            qw[v] = wrap_s ? qw0[v] : (wrap_c ? nqw : qw[v]);
            rw[v] = wrap_s ? rw0[v] : (wrap_c ? nrw : rw[v]);
            qh[v] = wrap_s ? nqh : qh[v];
            rh[v] = wrap_s ? nrh : rh[v];
        }
#pragma unroll
        for (int v = 0; v < kBV; ++v) {
            dma16(tile_ok ? sb[v] : zero, st + db[v]);
            sb[v] += step_b + (wrap_c ? next_tap_b : 0);
        }
        rq_stage = rq_stage + 1 == S ? 0 : rq_stage + 1;
        tap_c = wrap_c ? 0 : tap_c + kBK;
        tap_s = wrap_s ? 0 : tap_s + wrap_c;
        tap_r += wrap_s;
    };

    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int r = lane & 15, g = lane >> 4;
    int cp_stage = 0;
    auto compute = [&](int) __attribute__((always_inline)) {
        const unsigned char *ia = lds + cp_stage * kStage, *ib = ia + kAImg;
        cp_stage = cp_stage + 1 == S ? 0 : cp_stage + 1;
#pragma unroll
        for (int ks = 0; ks < kBK / 32; ++ks) {
            bf16x8 fa[WM], fb[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) fa[i] = ld_frag_rows(ia, wr * (BM / 4) + i * 16 + r, ks * 4 + g);
#pragma unroll
            for (int j = 0; j < WN; ++j) fb[j] = ld_frag_tr<BN * 2>(ib, wc * (BN / 2) + j * 16, ks * 32, lane);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
    };

#pragma unroll
    for (int kt = 0; kt < S - 1; ++kt) request();
    int kt = 0;
    for (; kt + S - 1 < nk; ++kt) {
        wait_and_barrier<(S - 2) * kPieces>();
        request();
        compute(kt);
    }
    drain<S - 2, kPieces>(kt, compute);

    store_tile<BM, BN>(acc, a.out, (long)a.Cin, nullptr, m0, n0, a.Min, a.Cin, wr, wc, r, g);
}

// ---- wgrad ------------------------------------------------------------------------------------------------------------------------------
template <int BM, int BN>
__global__ __launch_bounds__(kThreads) void conv2d_wgrad_kernel(const BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int kAImg = BM * kBK * 2;
    constexpr int kStage = Ring<BM, BN>::kStage, S = Ring<BM, BN>::kStages;
    constexpr int kAV = BM / 64, kBV = BN / 64;
    constexpr int kPieces = kAV + kBV;
    constexpr int WM = BM / 64, WN = BN / 32;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), wr = wave >> 1, wc = wave & 1;
    // the splits of one tile are a tile count apart: neighbours walk the same k range (the same pixels of gy and x)
    const int ntiles = a.tiles_m * a.tiles_n;
    const int split = (int)blockIdx.x / ntiles, tile = (int)blockIdx.x - split * ntiles;
    const int tn = tile / a.tiles_m, tm = tile - tn * a.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int NC = a.kh * a.kw * a.Cin;                                 // columns of the weight gradient
    const int kt0 = split * a.kper, kt1 = min(kt0 + a.kper, a.nkt);
    const int nk_real = kt1 - kt0;
    const int nk = nk_real > S - 1 ? nk_real : S - 1;
    const int pend = min(a.M, kt1 * kBK);                               // pixels from here on are not this split's: they read zeros

    const unsigned char *sa[kAV], *img[kBV];
    int rema[kAV], remb[kBV], ho[kBV], wo[kBV], offh[kBV], offw[kBV];
    uint32_t da[kAV], db[kBV];
    const unsigned char *zero = (const unsigned char *)kZeroRow + (lane & 7) * 16;
#pragma unroll
    for (int v = 0; v < kAV; ++v) {
        const int piece = v * 8 + wave;
        da[v] = piece * 1024;
        constexpr int RB = BM * 2, kPos = RB / 16;
        const int row = (piece * 64 + lane) / kPos, pos = (piece * 64 + lane) % kPos;
        const int ch = (((pos >> 1) ^ s_tr<RB>(row)) << 1) | (pos & 1);
        const int p = kt0 * kBK + row;
        rema[v] = pend - p;
        sa[v] = (const unsigned char *)(a.gy + (long)p * a.Cout + min(m0 + ch * 8, a.Cout - 8));
    }
    const long img_bytes = (long)a.H * a.W * a.Cin * 2;
#pragma unroll
    for (int v = 0; v < kBV; ++v) {
        const int piece = v * 8 + wave;
        db[v] = kAImg + piece * 1024;
        constexpr int RB = BN * 2, kPos = RB / 16;
        const int row = (piece * 64 + lane) / kPos, pos = (piece * 64 + lane) % kPos;
        const int ch = (((pos >> 1) ^ s_tr<RB>(row)) << 1) | (pos & 1);
        const int col = min(n0 + ch * 8, NC - 8);
        const int tap = col / a.Cin, c = col - tap * a.Cin, tr = tap / a.kw, ts = tap - tr * a.kw;
        offh[v] = tr * a.dh - a.ph;
        offw[v] = ts * a.dw - a.pw;
        const int p = kt0 * kBK + row;
        remb[v] = pend - p;
        const int n = p / (a.Ho * a.Wo), rem = p - n * (a.Ho * a.Wo);
        ho[v] = rem / a.Wo;
        wo[v] = rem - ho[v] * a.Wo;
        img[v] = (const unsigned char *)a.x + (long)n * img_bytes + c * 2;
    }
    // 64 pixels further: qn images, qh rows and qw columns, with a carry each
    const int hw = a.Ho * a.Wo;
    const int qn = kBK / hw, rem64 = kBK - qn * hw, qhh = rem64 / a.Wo, qww = rem64 - qhh * a.Wo;
    const long qn_bytes = (long)qn * img_bytes;
    const long step_a = (long)kBK * a.Cout * 2;
    const uint32_t l0 = lds_addr(lds);
    int rq_stage = 0;
    auto request = [&]() __attribute__((always_inline)) {
        const uint32_t st = l0 + rq_stage * kStage;
#pragma unroll
        for (int v = 0; v < kAV; ++v) {
            dma16(rema[v] > 0 ? sa[v] : zero, st + da[v]);
            sa[v] += step_a;
            rema[v] -= kBK;
        }
#pragma unroll
        for (int v = 0; v < kBV; ++v) {
            const int hi = ho[v] * a.sh + offh[v], wi = wo[v] * a.sw + offw[v];
            const bool ok = (remb[v] > 0) & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
            const unsigned pix = (unsigned)hi * (unsigned)a.W + (unsigned)wi;
            const unsigned char *px = img[v] + (unsigned long)pix * (unsigned)(a.Cin * 2);
            dma16(ok ? px : zero, st + db[v]);
            remb[v] -= kBK;
            int nw = wo[v] + qww;
            const int c1 = nw >= a.Wo;
            nw -= c1 ? a.Wo : 0;
            int nh = ho[v] + qhh + c1;
            const int c2 = nh >= a.Ho;
            nh -= c2 ? a.Ho : 0;
            wo[v] = nw;
            ho[v] = nh;
            img[v] += qn_bytes + (c2 ? img_bytes : 0);
        }
        rq_stage = rq_stage + 1 == S ? 0 : rq_stage + 1;
    };

    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int r = lane & 15, g = lane >> 4;
    int cp_stage = 0;
    auto compute = [&](int) __attribute__((always_inline)) {
        const unsigned char *ia = lds + cp_stage * kStage, *ib = ia + kAImg;
        cp_stage = cp_stage + 1 == S ? 0 : cp_stage + 1;
#pragma unroll
        for (int ks = 0; ks < kBK / 32; ++ks) {
            bf16x8 fa[WM], fb[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) fa[i] = ld_frag_tr<BM * 2>(ia, wr * (BM / 4) + i * 16, ks * 32, lane);
#pragma unroll
            for (int j = 0; j < WN; ++j) fb[j] = ld_frag_tr<BN * 2>(ib, wc * (BN / 2) + j * 16, ks * 32, lane);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
    };

#pragma unroll
    for (int kt = 0; kt < S - 1; ++kt) request();
    int kt = 0;
    for (; kt + S - 1 < nk; ++kt) {
        wait_and_barrier<(S - 2) * kPieces>();
        request();
        compute(kt);
    }
    drain<S - 2, kPieces>(kt, compute);

    if (a.ksplit > 1) {
        // ---- split-K hand-off (qt_linear_fqt.hip).  Partial sums leave in fragment order, write-through; every wave drains its stores;
        // behind the workgroup barrier ONE lane takes the tile's ticket.  Whoever draws the last ticket owns the tile: it adds ALL the
        // partial sums, its own included, in split order -- the result does not depend on who arrived last.  Nobody waits for anybody.
        constexpr long kSlab = (long)WM * WN * 256;                      // floats per wave
        float *const mine = a.ws + (((long)tile * a.ksplit + split) * 8 + wave) * kSlab;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) store16_sc1(mine + (i * WN + j) * 256, (uint32_t)lane * 16u, acc[i][j]);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();                                                // (also: every wave is done with the ring, the flag below reuses it)
        volatile unsigned int *flag = (volatile unsigned int *)lds;
        if (t == 0) *flag = __hip_atomic_fetch_add(a.tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if ((int)*flag != a.ksplit - 1) return;                         // not the last one: done
        if (t == 0) __hip_atomic_store(a.tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");              // drop what this XCD's L2 holds of the workspace from earlier launches
        const float *const base = a.ws + ((long)tile * a.ksplit * 8 + wave) * kSlab;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int q = 0; q < a.ksplit; ++q) {
            f32x4 part[WM][WN];
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) part[i][j] = load16_sc1(base + (long)q * 8 * kSlab + (i * WN + j) * 256, (uint32_t)lane * 16u);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) {
                    asm volatile("" : "+v"(part[i][j]));
                    acc[i][j] += part[i][j];
                }
        }
    }
    store_tile<BM, BN>(acc, a.out, (long)NC, nullptr, m0, n0, a.Cout, NC, wr, wc, r, g);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
// The geometry both products share with the forward (qt_conv.hip, conv_shape) and what each adds to it.
bool bwd_geometry(BwdArgs &a) {
    if (a.N < 1 || a.H < 1 || a.W < 1 || a.Cin < 8 || a.Cout < 8 || a.Cin % 8 != 0 || a.Cout % 8 != 0) return false;
    if (a.kh < 1 || a.kw < 1 || a.sh < 1 || a.sw < 1 || a.dh < 1 || a.dw < 1 || a.ph < 0 || a.pw < 0) return false;
    const long eh = (long)a.H + 2L * a.ph - (long)a.dh * (a.kh - 1) - 1, ew = (long)a.W + 2L * a.pw - (long)a.dw * (a.kw - 1) - 1;
    if (eh < 0 || ew < 0) return false;
    const long ho = eh / a.sh + 1, wo = ew / a.sw + 1, m = (long)a.N * ho * wo, min_ = (long)a.N * a.H * a.W;
    // 32-bit pixel indices; byte addresses are 64-bit
    if (m >= (1L << 30) || min_ >= (1L << 30) || (long)a.kh * a.dh >= (1 << 20) || (long)a.kw * a.dw >= (1 << 20) || a.ph >= (1 << 20) ||
        a.pw >= (1 << 20) || (long)a.kh * a.kw * a.Cin >= (1L << 30) || (long)a.kh * a.kw * a.Cout >= (1L << 30) || a.sh >= (1 << 20) || a.sw >= (1 << 20))
        return false;
    a.Ho = (int)ho; a.Wo = (int)wo; a.M = (int)m; a.Min = (int)min_;
    return true;
}

// dgrad: the forward's tile rule with the input pixels as rows and Cin as columns.
void dgrad_pick_tile(const BwdArgs &a, int &bm, int &bn) {
    const long cus = qt_cu_count();
    const long tm = (a.Min + 127) / 128;
    if (a.Cin >= 128 && tm * ((a.Cin + 127) / 128) >= cus) { bm = 128; bn = 128; }
    else if (tm * ((a.Cin + 63) / 64) * 2 >= cus) { bm = 128; bn = 64; }
    else { bm = 64; bn = 64; }
}

// wgrad: 128 x 128 tiles where they alone give every other CU a workgroup (the widest layers: 512 x 4608 is 144 tiles), else 64 x 64
// tiles.  The contraction is split until two workgroups per CU are in flight, a split keeping at least eight k tiles (512 pixels) so
// that the ring's fill and the hand-off stay small beside its work, 32 splits at the most (the owner reads every split's partial sums).
struct WgradPlan {
    int bm, bn, tiles_m, tiles_n, nkt, ksplit, kper;
    size_t ws_bytes() const { return ksplit > 1 ? (size_t)tiles_m * tiles_n * ksplit * bm * bn * 4 : 0; }
    size_t tickets() const { return ksplit > 1 ? (size_t)tiles_m * tiles_n : 0; }
};
WgradPlan wgrad_plan(const BwdArgs &a) {
    WgradPlan p{};
    const long cus = qt_cu_count();
    const long nc = (long)a.kh * a.kw * a.Cin;
    const long t128 = (long)((a.Cout + 127) / 128) * ((nc + 127) / 128);
    if (a.Cout >= 128 && t128 * 2 >= cus) { p.bm = 128; p.bn = 128; }
    else { p.bm = 64; p.bn = 64; }
    p.tiles_m = (a.Cout + p.bm - 1) / p.bm;
    p.tiles_n = (int)((nc + p.bn - 1) / p.bn);
    p.nkt = (a.M + kBK - 1) / kBK;
    const long tiles = (long)p.tiles_m * p.tiles_n;
    const long per_cu = p.bm == 128 ? 1 : 2;
    long want = per_cu * cus / tiles;
    if (want > 32) want = 32;
    if (want > p.nkt / 8) want = p.nkt / 8;
    if (want < 1) want = 1;
    p.kper = (int)((p.nkt + want - 1) / want);
    p.ksplit = (p.nkt + p.kper - 1) / p.kper;                            // (no empty split)
    return p;
}

template <int BM, int BN>
int dgrad_launch(BwdArgs &a, hipStream_t st) {
    constexpr int kLds = Ring<BM, BN>::kBytes;
    static_assert(kLds <= 160 * 1024, "the ring does not fit a CU's LDS");
    if (const int rc = qt_allow_lds<conv2d_dgrad_kernel<BM, BN>>(kLds)) return rc;
    conv2d_dgrad_kernel<BM, BN><<<(unsigned)(a.tiles_m * a.tiles_n), kThreads, kLds, st>>>(a);
    return qt_launch_status();
}

template <int BM, int BN>
int wgrad_launch(BwdArgs &a, hipStream_t st) {
    constexpr int kLds = Ring<BM, BN>::kBytes;
    static_assert(kLds <= 160 * 1024, "the ring does not fit a CU's LDS");
    if (const int rc = qt_allow_lds<conv2d_wgrad_kernel<BM, BN>>(kLds)) return rc;
    conv2d_wgrad_kernel<BM, BN><<<(unsigned)(a.tiles_m * a.tiles_n * a.ksplit), kThreads, kLds, st>>>(a);
    return qt_launch_status();
}

BwdArgs bwd_args(int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw) {
    BwdArgs a{};
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw; a.dh = dh; a.dw = dw;
    return a;
}

}  // namespace

extern "C" {

int qt_conv2d_backward_plan(int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                            qt_conv2d_product_plan *dgrad, qt_conv2d_product_plan *wgrad) {
    BwdArgs a = bwd_args(N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, dh, dw);
    const bool ok = bwd_geometry(a);
    if (dgrad) {
        *dgrad = qt_conv2d_product_plan{};
        if (ok && Cout % kBK == 0) {
            int bm, bn;
            dgrad_pick_tile(a, bm, bn);
            dgrad->taken = 1; dgrad->tile_m = bm; dgrad->tile_n = bn;
            dgrad->tiles_m = (a.Min + bm - 1) / bm; dgrad->tiles_n = (a.Cin + bn - 1) / bn;
            dgrad->k_tiles = kh * kw * (Cout / kBK);
            dgrad->ksplit = 1;
        }
    }
    if (wgrad) {
        *wgrad = qt_conv2d_product_plan{};
        if (ok) {
            const WgradPlan p = wgrad_plan(a);
            wgrad->taken = 1; wgrad->tile_m = p.bm; wgrad->tile_n = p.bn; wgrad->tiles_m = p.tiles_m; wgrad->tiles_n = p.tiles_n;
            wgrad->k_tiles = p.nkt; wgrad->ksplit = p.ksplit; wgrad->ws_bytes = p.ws_bytes(); wgrad->n_tickets = p.tickets();
        }
    }
    return ok ? QT_OK : QT_ERR_BAD_ARG;
}

int qt_conv2d_dgrad_bf16(const uint16_t *gy, const uint16_t *w, uint16_t *gx, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw,
                         int ph, int pw, int dh, int dw, void *stream) {
    BwdArgs a = bwd_args(N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, dh, dw);
    a.gy = gy; a.w = w; a.out = gx;
    if (!gy || !w || !gx || !bwd_geometry(a) || Cout % kBK != 0) return QT_ERR_BAD_ARG;
    if (((uintptr_t)gy | (uintptr_t)w) & 15u) return QT_ERR_UNALIGNED;
    if ((uintptr_t)gx & 7u) return QT_ERR_UNALIGNED;
    int bm, bn;
    dgrad_pick_tile(a, bm, bn);
    a.tiles_m = (a.Min + bm - 1) / bm;
    a.tiles_n = (a.Cin + bn - 1) / bn;
    hipStream_t st = (hipStream_t)stream;
    if (bm == 128 && bn == 128) return dgrad_launch<128, 128>(a, st);
    if (bm == 128) return dgrad_launch<128, 64>(a, st);
    return dgrad_launch<64, 64>(a, st);
}

int qt_conv2d_wgrad_bf16(const uint16_t *gy, const uint16_t *x, uint16_t *gw, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw,
                         int ph, int pw, int dh, int dw, float *ws, size_t ws_bytes, uint32_t *tickets, size_t n_tickets, void *stream) {
    BwdArgs a = bwd_args(N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, dh, dw);
    a.gy = gy; a.x = x; a.out = gw;
    if (!gy || !x || !gw || !bwd_geometry(a)) return QT_ERR_BAD_ARG;
    const WgradPlan p = wgrad_plan(a);
    if (p.ksplit > 1) {
        if (!ws || !tickets || ws_bytes < p.ws_bytes() || n_tickets < p.tickets()) return QT_ERR_BAD_ARG;
        if (((uintptr_t)ws & 15u) || ((uintptr_t)tickets & 3u)) return QT_ERR_UNALIGNED;
    }
    if (((uintptr_t)gy | (uintptr_t)x) & 15u) return QT_ERR_UNALIGNED;
    if ((uintptr_t)gw & 7u) return QT_ERR_UNALIGNED;
    a.tiles_m = p.tiles_m; a.tiles_n = p.tiles_n; a.ksplit = p.ksplit; a.kper = p.kper; a.nkt = p.nkt;
    a.ws = ws; a.tickets = tickets;
    hipStream_t st = (hipStream_t)stream;
    if (p.bm == 128) return wgrad_launch<128, 128>(a, st);
    return wgrad_launch<64, 64>(a, st);
}

}  // extern "C"
