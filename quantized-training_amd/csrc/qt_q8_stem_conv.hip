// The first convolution of a converted per-tensor int8 CNN (1 <= Cin <= 4: qt_q8_stem_conv2d*) on the integer matrix instruction.
// Epilogue, launch arguments and the checked shape of a launch: qt_mx_tile.h.
#include "qt_mx_tile.h"

namespace {

// ---- the stem as a patch kernel ------------------------------------------------------------------------------------------------------
// The gather kernel of qt_mx_conv.hip wants a 16-byte chunk inside one tap (Cin >= 32); a stem has 1 - 4 channels and many taps.  Here a
// pixel is ONE dword -- the codes pass qt_quantize_codes_nhwc4_* writes byte c = channel c, bytes >= Cin zero -- and the contraction
// runs in (r, s, c4) order with the filter row padded to kw' = 4 ceil(kw / 4) taps: a 16-byte "unit" u = r (kw' / 4) + q is the four
// neighbouring pixel dwords s = 4 q .. 4 q + 3 of filter row r.  v_mfma_i32_16x16x64_i8 takes one unit per lane (lane (row, g): k = 16 g
// + [0, 16) of the 64-deep step), so step t hands lane group g the unit 4 t + g, and the units are rounded up to whole steps.
//
// A workgroup (4 waves) owns patches of kStemPH x kStemPW = 8 x 16 output pixels of one image times one column tile of 16 NJ output
// channels (NJ = 2 for Cout <= 32, else 4), and walks the patches blockIdx.x, blockIdx.x + gridDim.x, ... so that its weight image is
// built once for several patches.  Per patch it stages the input halo -- ((8 - 1) sh + rows) x ((16 - 1) sw + kw') dwords -- into LDS
// once: a dword outside the plane, or in a halo row no real tap reaches, is zero; no address outside x is formed into a load.  The A
// fragment of output pixel (py, px), unit (r, q) is then the four dwords at halo[(py sh + r)][px sw + 4 q ..]: straight out of LDS,
// no per-element gather.  Wave w multiplies patch rows 2 w and 2 w + 1 (two 16-pixel row blocks) by the NJ column blocks.
//
// The weight arrives as stored for conv2d_q, int8 [Cout][kh][kw][Cin], and is padded into the LDS image [col][unit][4 taps][4 bytes]
// once per workgroup (no second copy in memory): taps s >= kw, rows r >= kh, channels >= Cin and columns >= Cout are ZERO WEIGHTS, so
// whatever the A side reads for them contributes exactly 0 to the int32 sum.  The halo allocation covers every such read: rows up to
// (8 - 1) sh + r_last where r_last is the filter row of the last padded unit.  The image's row pitch is 16 bytes more than the units,
// which spreads the sixteen columns of a B fragment read over the banks.
// Sums are exact: kh kw 4 <= 1024 products of magnitude <= 2^14, |sum| <= 2^24, and float(sum) is exact as well.
constexpr int kStemPH = 8, kStemPW = 16;
constexpr int kStemMaxTaps = 16;                       // kh, kw
constexpr int kStemLdsBudget = 96 * 1024;              // weight image + halo (or code tile), bytes
constexpr int kStemWgPerCu = 4;                        // patches are walked by at most this many workgroups per CU and column tile
constexpr int kStemCodePitch = 64 + 16;                // bytes of a code row of the CODES tile

struct StemGeom {
    int upr;                     // units per filter row, kw' / 4
    int nsteps;                  // 64-byte k steps
    int hw, hrows, hreal;        // halo width (dwords), rows allocated, rows a real tap reaches
    int pby, pbx, npatch;        // patches per image column / row, patches in all
    int wpitch;                  // bytes of one column of the weight image
    int halo_bytes;              // of the halo region (the CODES tile shares it)
    int cin;
};

template <int NJ, bool CODES>
__global__ __launch_bounds__(256) void q8_stem_kernel(MxGemmArgs a, MxConvGeom c, StemGeom s, tail_t<CODES> ct = {}) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint32_t *const halo = (uint32_t *)lds;
    uint8_t *const wimg = lds + s.halo_bytes;
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int r = l & 15, g = l >> 4;
    const int n0 = blockIdx.y * (16 * NJ);

    // the weight image of this column tile: destination dword d = (col, unit, tap of the unit)
    const int dwords_col = s.nsteps * 16;
    for (int d = t; d < 16 * NJ * dwords_col; d += 256) {
        const int col = d / dwords_col, k = d - col * dwords_col, u = k >> 2;
        const int fr = u / s.upr, fs = 4 * (u - fr * s.upr) + (k & 3);
        uint32_t v = 0u;
        if (n0 + col < a.N && fr < c.kh && fs < c.kw) {
            const uint8_t *src = a.B + ((long)(n0 + col) * (c.kh * c.kw) + fr * c.kw + fs) * s.cin;
            for (int ch = 0; ch < s.cin; ++ch) v |= (uint32_t)src[ch] << (8 * ch);
        }
        *(uint32_t *)(wimg + col * s.wpitch + 4 * k) = v;
    }

    // lane (r, g): the unit of step 0 and how a step moves it on
    const int d4r = 4 / s.upr, d4q = 4 - d4r * s.upr;
    const uint8_t *const wlane = wimg + r * s.wpitch + g * 16;
    const int pimg = s.pby * s.pbx;

    for (int p = blockIdx.x; p < s.npatch; p += gridDim.x) {
        const int n = p / pimg, pr = p - n * pimg, by = pr / s.pbx, bx = pr - by * s.pbx;
        const int ho0 = by * kStemPH, wo0 = bx * kStemPW;
        const int hi0 = ho0 * c.sh - c.ph, wi0 = wo0 * c.sw - c.pw;
        const uint32_t *const ximg = (const uint32_t *)a.A + (long)n * c.H * c.W;
        __syncthreads();                                  // the previous patch's last fragment (or code row) has been read
        for (int i = t; i < s.hrows * s.hw; i += 256) {
            const int hr = i / s.hw, hc = i - hr * s.hw;
            const int hi = hi0 + hr, wi = wi0 + hc;
            const bool ok = (hr < s.hreal) & ((unsigned)hi < (unsigned)c.H) & ((unsigned)wi < (unsigned)c.W);
            halo[i] = ok ? ximg[hi * c.W + wi] : 0u;
        }
        __syncthreads();

        v4i acc[2][NJ];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = v4i{0, 0, 0, 0};
        int tr = g / s.upr, tq = g - tr * s.upr;
        const uint32_t *const a0 = halo + (2 * w * c.sh) * s.hw + r * c.sw;
        const int a1 = c.sh * s.hw;
        for (int st = 0; st < s.nsteps; ++st) {
            const uint32_t *pa = a0 + tr * s.hw + 4 * tq;
            const v4i fa0 = {(int)pa[0], (int)pa[1], (int)pa[2], (int)pa[3]};
            const v4i fa1 = {(int)pa[a1], (int)pa[a1 + 1], (int)pa[a1 + 2], (int)pa[a1 + 3]};
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const v4i fb = *(const v4i *)(wlane + j * 16 * s.wpitch + st * 64);
                acc[0][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa0, fb, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa1, fb, acc[1][j], 0, 0, 0);
            }
            tr += d4r;
            tq += d4q;
            if (tq >= s.upr) { tq -= s.upr; ++tr; }
        }

        // epilogue: D col = l & 15 (+ 16 j), pixel of the row block = 4 g + e; y is [N Ho Wo][Cout]
        const long row0 = ((long)n * c.Ho + ho0) * c.Wo + wo0;
        if constexpr (CODES) {
            // a lane's bytes go into the patch's 128 x 16 NJ byte tile -- the halo's space, free behind the barrier -- and every thread
            // then writes whole 16-byte runs of a code row; pixels past the plane and runs >= Cout (Cout % 16 == 0) are skipped
            const float ns = next_scale_of(a, ct);
            __syncthreads();                              // every wave has read its last A fragment
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = n0 + j * 16 + r;
                if (col >= a.N) continue;
                const float bv = bias_of(a, col), sv = out_scale_of(a, col);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        lds[((2 * w + i) * kStemPW + 4 * g + e) * kStemCodePitch + j * 16 + r] =
                            (uint8_t)out_code(a, ct, ns, (float)acc[i][j][e], bv, sv);
            }
            __syncthreads();
            int8_t *y = (int8_t *)a.C;
            for (int q = t; q < kStemPH * kStemPW * NJ; q += 256) {
                const int px = q / NJ, run = q - px * NJ, py = px / kStemPW, pxx = px - py * kStemPW;
                if (ho0 + py >= c.Ho || wo0 + pxx >= c.Wo || n0 + run * 16 >= a.N) continue;
                *(uint4 *)(y + (row0 + (long)py * c.Wo + pxx) * a.N + n0 + run * 16) = *(const uint4 *)(lds + px * kStemCodePitch + run * 16);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = n0 + j * 16 + r;
                if (col >= a.N) continue;
                const float bv = bias_of(a, col), sv = out_scale_of(a, col);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int py = 2 * w + i;
                    if (ho0 + py >= c.Ho) continue;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int px = 4 * g + e;
                        if (wo0 + px >= c.Wo) continue;
                        emit_out(a, (float)acc[i][j][e], bv, sv, (row0 + (long)py * c.Wo + px) * a.N + col);
                    }
                }
            }
        }
    }
}

template <int NJ, bool CODES>
int launch_stem(const MxGemmArgs &g, const MxConvGeom &c, const StemGeom &s, int lds_bytes, hipStream_t st, const tail_t<CODES> &ct) {
    if (const int rc = qt_allow_lds<q8_stem_kernel<NJ, CODES>>(kStemLdsBudget)) return rc;
    const int tiles_n = (g.N + 16 * NJ - 1) / (16 * NJ);
    const long cap = (long)qt_cu_count() * kStemWgPerCu;
    const dim3 grid((unsigned)(s.npatch < cap ? s.npatch : cap), (unsigned)tiles_n);
    q8_stem_kernel<NJ, CODES><<<grid, 256, lds_bytes, st>>>(g, c, s, ct);
    return qt_launch_status();
}

int q8_stem_launch(const int8_t *x_codes, const int8_t *w_codes, void *y, int y_is_f32, const void *bias, const void *out_scale,
                   int out_scale_per_col, int fold_f32, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                   int dh, int dw, void *stream, const CodesTail *ct) {
    if (!x_codes || !w_codes || !y) return QT_ERR_BAD_ARG;
    if (ct) {
        if (const int rc = codes_tail_check(*ct, Cout < 0 ? 0 : Cout, y, y_is_f32)) return rc;
    }
    const bool rule = Cin >= 1 && Cin <= 4 && kh <= kStemMaxTaps && kw <= kStemMaxTaps && dh == 1 && dw == 1 && Cout % 16 == 0;
    const uintptr_t ptrs = (uintptr_t)x_codes | (uintptr_t)w_codes | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)out_scale;
    ConvShape cs;
    if (const int rc = conv_shape(N, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, rule ? QT_OK : QT_ERR_BAD_ARG, ptrs, Cin, 4, Cin, cs)) return rc;
    if (cs.empty) return QT_OK;
    const MxConvGeom &c = cs.c;
    const int nj = Cout <= 32 ? 2 : 4;
    StemGeom s;
    s.cin = Cin;
    s.upr = (kw + 3) / 4;
    const int units = kh * s.upr;
    s.nsteps = (units + 3) / 4;
    const int r_last = (4 * s.nsteps - 1) / s.upr;                        // the filter row of the last (padded) unit
    // halo extents in 64 bits: a stride may be anything below 2^20
    const long hw = (long)(kStemPW - 1) * sw + 4L * s.upr, hrows = (long)(kStemPH - 1) * sh + r_last + 1;
    long halo_bytes = hw * hrows * 4;
    if (ct && halo_bytes < kStemPH * kStemPW * kStemCodePitch) halo_bytes = kStemPH * kStemPW * kStemCodePitch;
    halo_bytes = (halo_bytes + 15) & ~15L;
    s.wpitch = s.nsteps * 64 + 16;
    const long lds_bytes = halo_bytes + 16L * nj * s.wpitch;
    if (lds_bytes > kStemLdsBudget) return QT_ERR_BAD_ARG;                 // the halo of this stride does not fit
    s.hw = (int)hw;
    s.hrows = (int)hrows;
    s.hreal = (kStemPH - 1) * sh + kh;
    s.halo_bytes = (int)halo_bytes;
    s.pby = (c.Ho + kStemPH - 1) / kStemPH;
    s.pbx = (c.Wo + kStemPW - 1) / kStemPW;
    const long npatch = mul_sat(N, mul_sat(s.pby, s.pbx));
    if (npatch >= kLim) return QT_ERR_BAD_ARG;
    s.npatch = (int)npatch;
    const uint8_t *A = (const uint8_t *)x_codes, *B = (const uint8_t *)w_codes;
    MxGemmArgs g{A, B, nullptr, nullptr, y, bias, (int)cs.m, Cout, (int)cs.taps * Cin, 0, 0, 0, 0, 0, y_is_f32, out_scale, out_scale_per_col, fold_f32};
    hipStream_t st = (hipStream_t)stream;
    if (ct) return nj == 2 ? launch_stem<2, true>(g, c, s, (int)lds_bytes, st, *ct) : launch_stem<4, true>(g, c, s, (int)lds_bytes, st, *ct);
    return nj == 2 ? launch_stem<2, false>(g, c, s, (int)lds_bytes, st, NoTail{}) : launch_stem<4, false>(g, c, s, (int)lds_bytes, st, NoTail{});
}

}  // namespace

extern "C" {

int qt_q8_stem_conv2d(const int8_t *x_codes4, const int8_t *w_codes, void *y, int y_is_f32, const void *bias, const void *out_scale,
                      int out_scale_per_col, int fold_f32, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph,
                      int pw, int dh, int dw, void *stream) {
    return q8_stem_launch(x_codes4, w_codes, y, y_is_f32, bias, out_scale, out_scale_per_col, fold_f32, N, H, W, Cin, Cout, kh,
                          kw, sh, sw, ph, pw, dh, dw, stream, nullptr);
}

int qt_q8_stem_conv2d_codes(const int8_t *x_codes4, const int8_t *w_codes, int8_t *y, int y_is_f32, const void *bias, const void *out_scale,
                            int out_scale_per_col, int fold_f32, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph,
                            int pw, int dh, int dw, int act, float act_lo, float act_hi, const void *next_scale, const uint16_t *next_qmap,
                            void *stream) {
    const CodesTail ct{next_qmap, next_scale, act, act_lo, act_hi};
    return q8_stem_launch(x_codes4, w_codes, y, y_is_f32, bias, out_scale, out_scale_per_col, fold_f32, N, H, W, Cin, Cout, kh,
                          kw, sh, sw, ph, pw, dh, dw, stream, &ct);
}

}  // extern "C"
