// qt_conv.hip -- Conv2d forward of a QAT convolution as an implicit GEMM on the matrix cores, in-tree.
//
// The reference's QAT Conv2d is self._conv_forward(input, self.weight_fake_quant(self.weight), self.bias) (modules/qat/conv.py:43-44, i.e.
// nn.Conv2d._conv_forward -> F.conv2d); ConvBn2d runs the same convolution on fq(weight * scale_factor) (conv_fused.py:103-126).  The weight
// arrives here already fake-quantized -- bf16 VALUES; this kernel does not quantize:
//     y[n, ho, wo, co] = sum over (r, s, c) of x[n, ho sh - ph + r dh, wo sw - pw + s dw, c] . wq[co, r, s, c]  (+ bias[co])
// bf16 NHWC activations, [Cout][kh][kw][Cin] weights, fp32 accumulation on v_mfma_f32_16x16x32_bf16, bias added in fp32, ONE rounding to
// bf16, written NHWC = [M][Cout] with M = N Ho Wo.  The summation order of an output element is fixed by the tile walk -- taps in (r, s)
// order, channel chunks of 64 ascending, 32 products per matrix instruction --: the same bits on every launch.
//
// GEMM view.  Rows = output pixels, columns = Cout, K = kh kw Cin walked in k tiles of 64 channels of ONE tap.  The weight operand is the
// forward layout of qt_train_gemm.hip (B = [N][K], k contiguous) as it stands.  The activation operand has no matrix in memory: row m of k
// tile (r, s, c0) is the 128 contiguous bytes x[n, hi, wi, c0 : c0 + 64] of the input pixel the tap points at.  LDS-DMA takes a source
// address PER LANE (dma16), so the [rows][64 k] image of the ring is filled by a gather: a wave's piece is 8 rows x 8 chunks of 16 bytes,
// lane l fetches chunk (l & 7) ^ swizzle(row) of row l >> 3 (the XOR swizzle goes on the SOURCE chunk, the DMA writes the piece linearly).
// A row whose tap falls into the zero padding, a row past M in the ragged last row tile, and the tiles that pad a short contraction up to
// the ring's depth point their lanes at a 128-byte block of zeros instead -- chosen by a select, no branch in the k step.
// A lane's (n, ho sh - ph, wo sw - pw) do not change over the k loop: they are computed once, and a k tile adds the tap's offset.
// Ring, image offsets, fragment read, drain and epilogue: qt_gemm_ring.h, shared with qt_train_gemm.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_gemm_ring.h"

namespace {

__device__ __attribute__((aligned(128))) const uint32_t kZeroRow[32] = {0};      // what padding taps and rows past M read

struct ConvArgs {
    const uint16_t *x, *w, *bias;
    uint16_t *y;
    int N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, dh, dw;
    int Ho, Wo, M;
    int tiles_m, tiles_n;
};

template <int BM, int BN>
__global__ __launch_bounds__(kThreads) void conv2d_kernel(const ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int kAImg = BM * kBK * 2;
    constexpr int kStage = Ring<BM, BN>::kStage, S = Ring<BM, BN>::kStages;
    constexpr int kAV = BM / 64, kBV = BN / 64;                         // DMA pieces (1 KiB) per wave and k tile
    constexpr int kPieces = kAV + kBV;
    constexpr int WM = BM / 64, WN = BN / 32;                           // 16 x 16 output tiles per wave: the wave owns (BM / 4) x (BN / 2)
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), wr = wave >> 1, wc = wave & 1;
    // consecutive workgroups walk the row tiles of one column tile (xcd_run: an XCD's L2 then holds a contiguous band of the activations)
    const int total = a.tiles_m * a.tiles_n;
    const int tile = (a.tiles_m & 7) ? xcd_run((int)blockIdx.x, total) : (int)blockIdx.x;
    const int tn = tile / a.tiles_m, tm = tile % a.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nk_real = a.kh * a.kw * (a.Cin / kBK);
    const int nk = nk_real > S - 1 ? nk_real : S - 1;                   // a 1 x 1 filter over 64 channels is ONE k tile: zero tiles fill the ring

    // ---- the address generator.  Per lane and activation piece: the pixel the filter's corner sits on and that pixel's address (+ the
    // swizzled chunk); rows past M get a corner no tap brings back into the plane.
    const unsigned char *pa[kAV], *sb[kBV];
    int hi0[kAV], wi0[kAV];
    uint32_t da[kAV], db[kBV];
    const unsigned char *zero = (const unsigned char *)kZeroRow + (lane & 7) * 16;
#pragma unroll
    for (int v = 0; v < kAV; ++v) {
        const int piece = v * 8 + wave;
        da[v] = piece * 1024;
        const int row = piece * 8 + (lane >> 3), pos = lane & 7, ch = pos ^ ((row >> 1) & 7);
        const int m = m0 + row, live = m < a.M;
        const int mm = live ? m : 0;
        const int n = mm / (a.Ho * a.Wo), rem = mm - n * (a.Ho * a.Wo), ho = rem / a.Wo, wo = rem - ho * a.Wo;
        hi0[v] = live ? ho * a.sh - a.ph : -(1 << 28);
        wi0[v] = wo * a.sw - a.pw;
        // (the corner's own address, possibly outside the plane: only taps that land inside it are fetched)
        pa[v] = (const unsigned char *)(a.x + ((long)n * a.H * a.W + (long)hi0[v] * a.W + wi0[v]) * a.Cin) + ch * 16;
    }
#pragma unroll
    for (int v = 0; v < kBV; ++v) {
        const int piece = v * 8 + wave;
        db[v] = kAImg + piece * 1024;
        const int row = piece * 8 + (lane >> 3), pos = lane & 7, ch = pos ^ ((row >> 1) & 7);
        sb[v] = (const unsigned char *)(a.w + (long)min(n0 + row, a.Cout - 1) * a.kh * a.kw * a.Cin + ch * 8);
    }
    const uint32_t l0 = lds_addr(lds);
    int rq_stage = 0;
    // the k tile the next request fetches (wave-uniform): tap (r, s), channel chunk c; kept as what the tap adds to a corner's row, column
    // and address, and moved on by additions only -- channel chunks ascending inside a tap, taps in (r, s) order
    int tap_r = 0, tap_s = 0, tap_c = 0, dr = 0, ds = 0;
    long tap_off = 0;                                                   // ((r dh W + s dw) Cin + c) * 2
    const long next_s = (long)(a.dw - 1) * a.Cin * 2, next_r = ((long)a.dh * a.W - (long)a.kw * a.dw) * a.Cin * 2;
    auto request = [&]() __attribute__((always_inline)) {
        const uint32_t st = l0 + rq_stage * kStage;
        const bool tile_ok = tap_r < a.kh;                              // (false for the zero tiles behind a short contraction)
#pragma unroll
        for (int v = 0; v < kAV; ++v) {
            const int hi = hi0[v] + dr, wi = wi0[v] + ds;
            const bool ok = tile_ok & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
            const unsigned char *px = pa[v] + tap_off;
            dma16(ok ? px : zero, st + da[v]);
        }
#pragma unroll
        for (int v = 0; v < kBV; ++v) {
            dma16(tile_ok ? sb[v] : zero, st + db[v]);
            sb[v] += kBK * 2;
        }
        rq_stage = rq_stage + 1 == S ? 0 : rq_stage + 1;
        tap_c += kBK;
        const bool wrap_c = tap_c == a.Cin;
        tap_c = wrap_c ? 0 : tap_c;
        tap_s += wrap_c;
        const bool wrap_s = tap_s == a.kw;
        tap_s = wrap_s ? 0 : tap_s;
        tap_r += wrap_s;
        ds = wrap_s ? 0 : ds + (wrap_c ? a.dw : 0);
        dr += wrap_s ? a.dh : 0;
        tap_off += kBK * 2 + (wrap_c ? next_s : 0) + (wrap_s ? next_r : 0);
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
            for (int j = 0; j < WN; ++j) fb[j] = ld_frag_rows(ib, wc * (BN / 2) + j * 16 + r, ks * 4 + g);
            // operands swapped: a lane then owns four consecutive output channels of one pixel (an 8-byte store)
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
    };

    // ---- k loop, as in qt_train_gemm.hip: S - 1 k tiles in flight, one barrier per k tile
#pragma unroll
    for (int kt = 0; kt < S - 1; ++kt) request();
    int kt = 0;
    for (; kt + S - 1 < nk; ++kt) {
        wait_and_barrier<(S - 2) * kPieces>();
        request();
        compute(kt);
    }
    drain<S - 2, kPieces>(kt, compute);

    store_tile<BM, BN>(acc, a.y, (long)a.Cout, a.bias, m0, n0, a.M, a.Cout, wr, wc, r, g);
}

// What the kernel takes (anything else: QT_ERR_BAD_ARG, the caller keeps the library's convolution), and the derived sizes.
bool conv_shape(ConvArgs &a) {
    if (a.N < 1 || a.H < 1 || a.W < 1 || a.Cin < kBK || a.Cin % kBK != 0 || a.Cout < 8 || a.Cout % 8 != 0) return false;
    if (a.kh < 1 || a.kw < 1 || a.sh < 1 || a.sw < 1 || a.dh < 1 || a.dw < 1 || a.ph < 0 || a.pw < 0) return false;
    const long eh = (long)a.H + 2L * a.ph - (long)a.dh * (a.kh - 1) - 1, ew = (long)a.W + 2L * a.pw - (long)a.dw * (a.kw - 1) - 1;
    if (eh < 0 || ew < 0) return false;
    const long ho = eh / a.sh + 1, wo = ew / a.sw + 1, m = (long)a.N * ho * wo;
    // 32-bit pixel indices inside one image and inside the output; byte addresses are 64-bit
    if (m >= (1L << 30) || (long)a.H * a.W >= (1L << 30) || (long)a.kh * a.dh >= (1 << 20) || (long)a.kw * a.dw >= (1 << 20) || a.ph >= (1 << 20) ||
        a.pw >= (1 << 20) || (long)a.kh * a.kw * a.Cin >= (1L << 30))
        return false;
    a.Ho = (int)ho; a.Wo = (int)wo; a.M = (int)m;
    return true;
}

// Tile choice: qt_train_gemm.hip's rule for k-contiguous operands (128 x 64 tiles, two workgroups per CU, where they give at least half a
// workgroup per CU; else 64 x 64), and 128 x 128 tiles where Cout is at least 128 and they still give every CU a tile: the gathered
// activation tile -- the operand that is re-fetched once per column tile -- is then read half as often (measured table).
void conv_pick_tile(const ConvArgs &a, int &bm, int &bn) {
    const long cus = qt_cu_count();
    const long tm = (a.M + 127) / 128;
    if (a.Cout >= 128 && tm * ((a.Cout + 127) / 128) >= cus) { bm = 128; bn = 128; }
    else if (tm * ((a.Cout + 63) / 64) * 2 >= cus) { bm = 128; bn = 64; }
    else { bm = 64; bn = 64; }
}

template <int BM, int BN>
int conv_launch(ConvArgs &a, hipStream_t st) {
    constexpr int kLds = Ring<BM, BN>::kBytes;
    static_assert(kLds <= 160 * 1024, "the ring does not fit a CU's LDS");
    if (const int rc = qt_allow_lds<conv2d_kernel<BM, BN>>(kLds)) return rc;
    conv2d_kernel<BM, BN><<<(unsigned)(a.tiles_m * a.tiles_n), kThreads, kLds, st>>>(a);
    return qt_launch_status();
}

}  // namespace

extern "C" {

int qt_conv2d_plan(int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int *tile_m, int *tile_n,
                   int *tiles_m, int *tiles_n, int *k_tiles) {
    ConvArgs a{};
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw; a.dh = dh; a.dw = dw;
    if (!conv_shape(a)) return QT_ERR_BAD_ARG;
    int bm, bn;
    conv_pick_tile(a, bm, bn);
    if (tile_m) *tile_m = bm;
    if (tile_n) *tile_n = bn;
    if (tiles_m) *tiles_m = (a.M + bm - 1) / bm;
    if (tiles_n) *tiles_n = (a.Cout + bn - 1) / bn;
    if (k_tiles) *k_tiles = kh * kw * (Cin / kBK);
    return QT_OK;
}

int qt_conv2d_bf16(const uint16_t *x, const uint16_t *w, const uint16_t *bias, uint16_t *y, int N, int H, int W, int Cin, int Cout, int kh, int kw,
                   int sh, int sw, int ph, int pw, int dh, int dw, void *stream) {
    ConvArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw; a.dh = dh; a.dw = dw;
    if (!x || !w || !y || !conv_shape(a)) return QT_ERR_BAD_ARG;
    if (((uintptr_t)x | (uintptr_t)w) & 15u) return QT_ERR_UNALIGNED;
    if (((uintptr_t)y | (uintptr_t)bias) & 7u) return QT_ERR_UNALIGNED;
    int bm, bn;
    conv_pick_tile(a, bm, bn);
#ifdef QT_TUNING_BUILD
    if (const char *e = getenv("QT_CONV_TILE")) {                       // tools/ only: "128x64"
        int fm = 0, fn = 0;
        if (sscanf(e, "%dx%d", &fm, &fn) == 2 && ((fm == 128 && (fn == 64 || fn == 128)) || (fm == 64 && fn == 64))) { bm = fm; bn = fn; }
    }
#endif
    a.tiles_m = (a.M + bm - 1) / bm;
    a.tiles_n = (a.Cout + bn - 1) / bn;
    hipStream_t st = (hipStream_t)stream;
    if (bm == 128 && bn == 128) return conv_launch<128, 128>(a, st);
    if (bm == 128) return conv_launch<128, 64>(a, st);
    return conv_launch<64, 64>(a, st);
}

}  // extern "C"
