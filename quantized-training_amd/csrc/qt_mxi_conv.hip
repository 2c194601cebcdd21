// conv2d_mx for integer and codebook operands under arbitrary block scales (qt_conv2d_mxi): the implicit GEMM of qt_mx_conv.hip on the
// arithmetic of qt_mxi_gemm.hip.
//
// Rows = output pixels (n, ho, wo), columns = Cout, K = kh kw Cin ordered (r, s, c); blocks of BS channels, Cin % BS == 0, so a block
// never straddles a filter tap.  Operands as qt_mxi_pack leaves them: x codes NHWC [N][H][W][Cin] int8 with fp32 scales
// [N][H][W][Cin / BS]; w codes [Cout][kh][kw][Cin] with scales [Cout][kh][kw][Cin / BS].
//     y[n, ho, wo, co] = rd( bias[co] + sum_{(r, s, kb)} (sx[n, hi, wi, kb] sw[co, r, s, kb]) * p ),   p = sum_{c in block kb} x[n, hi, wi, c] w[co, r, s, c]
// p is one block on the integer matrix cores, exact in int32 and in its conversion to fp32; t = sx * sw is one fp32 product;
// acc = fma(p, t, acc) in increasing virtual k; bias added in fp32, one rounding.  No atomics, no split of K: the same bits on every launch.
//
// The register-staged, double-buffered 128 x 128 x 128 kernel, one instantiation per BS:
//   * A codes: mx_conv_kernel's gather at one byte per element (P = Cin bytes per pixel): a corner per staged chunk, the wave-uniform
//     tap state (u_blk, u_ts, u_tr) moved on by additions, zero chunks for padding taps, rows >= M and the K tail, whose loads are
//     redirected to byte 0 of the operand;
//   * A scales: the thread that stages tile row t (t < 128) owns that row's output pixel.  Block q of the k tile starts at 32-block
//     u_blk + q BS / 32 counted from the tile's first tap; conv_tap_of gives its tap and its place inside the tap, the scale is
//     x_scales[pixel(tap) Cin / BS + place / (BS / 32)].  A dead block (padding, row >= M, K tail) loads element 0 and stores 0.f:
//     its codes are zero chunks, so the term is fma(0, 0 * sw, acc) = acc;
//   * B codes and scales (threads 128-255 stage the scales of tile row t - 128): dense rows of kh kw Cin bytes, as in mxi_gemm_kernel;
//   * the products: mxi_gemm_kernel's, from the same LDS image -- codes in Tile<0>, scales as s[operand][block][row].
// Both halves of the workgroup run the same instructions in the k loop (the scale address and its liveness are selected, not
// branched on), so the loop stays one basic block between its scheduling fences.
#include "qt_mx_tile.h"

namespace {

template <int BS>
__global__ __launch_bounds__(256) void mxi_conv_kernel(MxGemmArgs a, MxConvGeom c) {
    using T = Tile<0>;
    constexpr int NS = Mxi<BS>::kScales;
    constexpr int U = BS / 32;                                    // 32-blocks per scale block
    constexpr int R = T::kRow, CH = T::kChunks;                   // 128 bytes, 8 chunks per tile row
    constexpr int NC = kBM * CH / 256;                            // chunks per thread and operand
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    auto s_a = [&](int buf) __attribute__((always_inline)) { return lds + buf * T::kBytes; };
    auto s_b = [&](int buf) __attribute__((always_inline)) { return lds + 2 * T::kBytes + buf * T::kBytes; };
    auto s_s = [&](int buf) __attribute__((always_inline)) { return (float *)(lds + 4 * T::kBytes) + buf * Mxi<BS>::kScaleFloats; };

    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int r = l & 15, g = l >> 4;
    const int wm = w >> 1, wn = w & 1;
    const int tiles_m = (a.M + kBM - 1) / kBM, tiles_n = (a.N + kBN - 1) / kBN;
    const TileAt at = tile_at<kBM, kBN, 8>(tiles_m * tiles_n, tiles_m, tiles_n, blockIdx.x);
    const int m0 = at.m0, n0 = at.n0;
    const int nblk = a.K / BS;
    const int nk = (a.K + kBK - 1) / kBK;
    const int pbytes = c.cpb * 32;                                // P: code bytes of one input pixel
    const int spp = c.cpb / U;                                    // scales of one input pixel
    const long kb_row = a.K;                                      // bytes per weight row

    // an output pixel's input corner (mx_conv_kernel): the pixel index it would have (modulo 2^32: only taps inside the plane are
    // fetched) and its row / column; rows past M get a corner that no tap brings back into the plane
    auto corner = [&](int m, uint32_t &pix, int &hi0, int &wi0) __attribute__((always_inline)) {
        const bool live = m < a.M;
        const int mm = live ? m : 0;
        const int n = mm / (c.Ho * c.Wo), rem = mm - n * (c.Ho * c.Wo), ho = rem / c.Wo, wo = rem - ho * c.Wo;
        hi0 = live ? ho * c.sh - c.ph : -(1 << 28);
        wi0 = wo * c.sw - c.pw;
        pix = (uint32_t)n * (uint32_t)(c.H * c.W) + (uint32_t)hi0 * (uint32_t)c.W + (uint32_t)wi0;
    };
    uint32_t ga[NC];                 // byte offsets of the corners into x_codes
    int hia[NC], wia[NC];
    const uint8_t *gb[NC];
    int la[NC], ca[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int ch = t + 256 * i, row = ch / CH, cc = ch % CH;
        uint32_t pix;
        corner(m0 + row, pix, hia[i], wia[i]);
        ga[i] = pix * (uint32_t)pbytes;
        gb[i] = a.B + (long)min(n0 + row, a.N - 1) * kb_row + cc * 16;
        la[i] = T::chunk_off(row, cc);
        ca[i] = cc * 16;
    }
    // thread (operand t >> 7, tile row t & 127) stages that row's block scales of the k tile: operand 0 through its pixel's corner
    const int sop = t >> 7, srow = t & 127;
    uint32_t spix;
    int his, wis;
    corner(m0 + srow, spix, his, wis);
    const uint32_t gs = spix * (uint32_t)spp;                     // element offset of the corner into x_scales
    const float *xs = (const float *)a.sA;
    const float *ps = (const float *)a.sB + (long)min(n0 + srow, a.N - 1) * nblk;

    uint4 ra[NC], rb[NC];
    bool oka[NC], oks[NS];
    float rs[NS];
    int u_blk = 0, u_ts = 0, u_tr = 0;                            // where the next k tile to load starts: 32-block u_blk of tap (u_tr, u_ts)
    auto load_tile = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            int off, ts, tr;
            conv_tap_of(u_blk * 32 + ca[i], pbytes, u_ts, u_tr, c.kw, off, ts, tr);
            const int hi = hia[i] + tr * c.dh, wi = wia[i] + ts * c.dw;
            oka[i] = (tr < c.kh) & ((unsigned)hi < (unsigned)c.H) & ((unsigned)wi < (unsigned)c.W);    // tr >= kh: the K tail
            const uint32_t src = ga[i] + ((uint32_t)(tr * c.dh) * (uint32_t)c.W + (uint32_t)(ts * c.dw)) * (uint32_t)pbytes + (uint32_t)off;
            ra[i] = *(const uint4 *)(a.A + (oka[i] ? src : 0u));
            // the k tail re-reads chunk 0 of the weight row; it is replaced by zeros when it is stored
            const long koff = (long)kt * R + ca[i];
            rb[i] = *(const uint4 *)(gb[i] + (koff < kb_row ? (long)kt * R : -(long)ca[i]));
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            int blk, ts, tr;
            conv_tap_of(u_blk + q * U, c.cpb, u_ts, u_tr, c.kw, blk, ts, tr);
            const int hi = his + tr * c.dh, wi = wis + ts * c.dw;
            const bool ok = (tr < c.kh) & ((unsigned)hi < (unsigned)c.H) & ((unsigned)wi < (unsigned)c.W);
            const uint32_t src = gs + ((uint32_t)(tr * c.dh) * (uint32_t)c.W + (uint32_t)(ts * c.dw)) * (uint32_t)spp + (uint32_t)(blk / U);
            const float *pa = xs + (ok ? src : 0u);
            const float *pb = ps + min(kt * NS + q, nblk - 1);
            rs[q] = *(sop ? pb : pa);
            oks[q] = sop ? kt * NS + q < nblk : ok;
        }
        int nb, ns, nr;
        conv_tap_of(u_blk + 4, c.cpb, u_ts, u_tr, c.kw, nb, ns, nr);
        u_blk = nb; u_ts = ns; u_tr = nr;
    };
    auto store_tile = [&](int buf, int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            *(uint4 *)(s_a(buf) + la[i]) = chunk_or_zero(oka[i], ra[i]);
            *(uint4 *)(s_b(buf) + la[i]) = chunk_or_zero((long)kt * R + ca[i] < kb_row, rb[i]);
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) s_s(buf)[(sop * NS + q) * 128 + srow] = oks[q] ? rs[q] : 0.f;
    };

    v4f acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](int cur) __attribute__((always_inline)) {
        const float *ss = s_s(cur);
        v8i fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (BS == 32) {
                fa[i] = read_frag32(s_a(cur), wm * 64 + i * 16 + r, g);
                fb[i] = read_frag32(s_b(cur), wn * 64 + i * 16 + r, g);
            } else {
                fa[i] = read_frag<0>(s_a(cur), wm * 64 + i * 16 + r, g);
                fb[i] = read_frag<0>(s_b(cur), wn * 64 + i * 16 + r, g);
            }
        }
#pragma unroll
        for (int blk = 0; blk < NS; ++blk) {                      // increasing virtual k
            v4f sa[4];
            float sb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sa[i] = *(const v4f *)(ss + blk * 128 + wm * 64 + i * 16 + 4 * g);       // rows 4 g + e of fragment tile i
                sb[i] = ss[(NS + blk) * 128 + wn * 64 + i * 16 + r];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const v4i p = mxi_block<BS>(fa[i], fb[j], blk);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][j][e] = __builtin_fmaf((float)p[e], sa[i][e] * sb[j], acc[i][j][e]);
                }
        }
    };

    load_tile(0);
    store_tile(0, 0);
    __syncthreads();
    for (int kt = 0; kt + 1 < nk; ++kt) {
        const int cur = kt & 1;
        load_tile(kt + 1);                                // in flight during this tile's products
        __builtin_amdgcn_sched_barrier(0);
        compute(cur);
        __builtin_amdgcn_sched_barrier(0);
        store_tile(cur ^ 1, kt + 1);
        __syncthreads();
    }
    compute((nk - 1) & 1);

    // epilogue: D col = l & 15, row = 4 g + e; y is [M][Cout] = NHWC
    emit_tile<false>(a, acc, m0 + wm * 64, n0 + wn * 64, 0L, r, g);
}

template <int BS>
int launch_mxi_conv(const MxGemmArgs &g, const MxConvGeom &c, unsigned grid, hipStream_t st) {
    if (const int rc = qt_allow_lds<mxi_conv_kernel<BS>>(Mxi<BS>::kLds)) return rc;
    mxi_conv_kernel<BS><<<grid, 256, Mxi<BS>::kLds, st>>>(g, c);
    return qt_launch_status();
}

}  // namespace

extern "C" {

int qt_conv2d_mxi(const int8_t *x_codes, const float *x_scales, const int8_t *w_codes, const float *w_scales, int block_size, void *y,
                  int y_is_f32, const void *bias, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                  int dh, int dw, void *stream) {
    if (!x_codes || !x_scales || !w_codes || !w_scales || !y) return QT_ERR_BAD_ARG;
    if (block_size != 32 && block_size != 64 && block_size != 128) return QT_ERR_BAD_ARG;
    if (Cin < block_size || Cin % block_size != 0 || Cin > (1 << 24)) return QT_ERR_BAD_ARG;
    // one byte per element: the code arrays are bounded through conv_shape's byte limits, the scale arrays are smaller
    ConvShape s;
    if (const int rc = conv_shape(N, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, QT_OK, (uintptr_t)x_codes | (uintptr_t)w_codes, Cin, Cin, Cin, s))
        return rc;
    if (s.empty) return QT_OK;
    const uintptr_t elem = y_is_f32 ? 3u : 1u;
    if ((((uintptr_t)x_scales | (uintptr_t)w_scales) & 3u) || (((uintptr_t)y | (uintptr_t)bias) & elem)) return QT_ERR_UNALIGNED;
    const long tiles = ((s.m + kBM - 1) / kBM) * ((Cout + kBN - 1) / kBN);
    if (tiles >= kLim) return QT_ERR_BAD_ARG;
    const int K = (int)(s.taps * Cin);
    MxGemmArgs g{(const uint8_t *)x_codes, (const uint8_t *)w_codes, (const uint8_t *)x_scales, (const uint8_t *)w_scales, y, bias,
                 (int)s.m, Cout, K, 0, 0, 0, 0, 0, y_is_f32, nullptr, 0, 0};
    s.c.cpb = Cin / 32;
    hipStream_t st = (hipStream_t)stream;
    if (block_size == 32) return launch_mxi_conv<32>(g, s.c, (unsigned)tiles, st);
    if (block_size == 64) return launch_mxi_conv<64>(g, s.c, (unsigned)tiles, st);
    return launch_mxi_conv<128>(g, s.c, (unsigned)tiles, st);
}

}  // extern "C"
